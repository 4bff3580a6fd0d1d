"""-m gpu: scores of the text decoder -- loco_decoder_score (csrc/decoder_score.hip) and what is built on it: forward(labels=), score,
score_many, generate(output_scores=True, return_dict_in_generate=True), generate_many(return_scores=True), transcribe --scores.

1. the operator against float64 log_softmax of the same fp32 logits          5. the pool: scores do not depend on the neighbours, bitwise
2. row independence, bitwise                                                 6. score_many against score per pair
3. forward(labels=) against the float64 decoder oracle                       7. the CLI
4. generate with scores

The operator's bar per element is max(4 e_torch, 2^-21 max(1, |ref|)): e_torch is the largest error of torch's own CPU fp32
log_softmax against float64 at the case's scored elements (the reference's error, never the kernel's; the 4 allows another summation
order and another expf), the floor is 4 ulp of the result.  Sums are accumulated in double on the device and stored as fp32, so a
sum is held to the sum of its tokens' bars plus the store's rounding, 2^-24 |sum|."""
import importlib
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_pool_cases as pc
import decoder_sweep_cases as cases
import speecht5_decoder_oracle as dec_oracle
from conftest import golden, record_figure
from test_gpu_decoder import full_model
from test_gpu_decoder_pool import batches_of, encode, small_model

pytestmark = pytest.mark.gpu

IGNORE = -100
GAP = 1e30  # what the columns between V and ld hold: read once, it would show in every sum


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def dec():
    return importlib.import_module("loco-asr_amd.decoder")


def floor_of(ref):
    return 2.0 ** -21 * torch.clamp(torch.as_tensor(ref, dtype=torch.float64).abs(), min=1.0)


def score_op(gu, rows, V, B, S, targets=None, chosen=False, reduce=True):
    """loco_decoder_score on ``rows`` f32 [B * S, ld] (host): dict of host tensors lp [B, S], seq [B], cnt [B], loss (float), chosen."""
    M, ld = rows.shape
    assert M == B * S and ld >= V
    x = gu.dev(rows)
    t = gu.dev(targets, torch.int32) if targets is not None else None
    lp = torch.full((B, S), 123.0, device="cuda")
    ch = torch.full((B, S), -7, dtype=torch.int32, device="cuda") if chosen else None
    seq = torch.full((B,), 123.0, device="cuda") if reduce else None
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda") if reduce else None
    loss = torch.full((1,), 123.0, device="cuda") if reduce else None
    gu.check(gu.lib().loco_decoder_score(gu.ptr(x), ld, gu.ptr(t), B, S, V, IGNORE, gu.ptr(lp), gu.ptr(ch), gu.ptr(seq), gu.ptr(cnt), gu.ptr(loss),
                                         gu.stream()), "loco_decoder_score")
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(torch.int32), torch.as_tensor(rows).contiguous().view(torch.int32))  # the logits are only read (bits: NaN rows)
    c = lambda v: v.cpu() if v is not None else None  # noqa: E731
    return dict(lp=c(lp), seq=c(seq), cnt=c(cnt), loss=float(loss[0]) if reduce else None, chosen=c(ch))


def padded(x, ld):
    """[M, V] -> [M, ld] with GAP in the columns a kernel must never read."""
    out = torch.full((x.shape[0], ld), GAP, dtype=torch.float32)
    out[:, :x.shape[1]] = x
    return out


def reference(x, targets):
    """(float64 log-probability at the targets -- 0 where ignored --, e_torch over the scored elements, torch fp32's own values)."""
    V = x.shape[1]
    t = torch.as_tensor(targets).long()
    valid = t != IGNORE
    idx = t.clamp(0, V - 1)[:, None]
    ref = torch.log_softmax(x.double(), -1).gather(1, idx)[:, 0] * valid
    own = torch.log_softmax(x, -1).gather(1, idx)[:, 0] * valid
    ref, own = torch.where(valid, ref, torch.zeros((), dtype=torch.float64)), torch.where(valid, own, torch.zeros(()))
    fin = torch.isfinite(ref)
    e_torch = float((own.double() - ref)[fin].abs().max()) if bool(fin.any()) else 0.0
    return ref, e_torch, own


def check_tokens(got, ref, e_torch, own):
    """Worst error / bar over the finite elements; non-finite results exactly where torch's own are, and the same ones."""
    got, fin = got.flatten().double(), torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(own)), (got, own)
    assert torch.equal(got[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)])  # -inf stays -inf
    bar = torch.maximum(torch.full_like(ref, 4 * e_torch), floor_of(ref))
    ratio = ((got - ref).abs() / bar)[fin]
    return (float(ratio.max()) if ratio.numel() else 0.0), bar


def check_sums(out, ref, bar, targets, B, S):
    """seq_logprob, seq_count and loss against float64 sums of the reference's per-token values (finite references only)."""
    valid = (torch.as_tensor(targets).long() != IGNORE).view(B, S)
    ref, bar = ref.view(B, S), bar.view(B, S) * valid
    assert out["cnt"].tolist() == valid.sum(1).tolist()
    want = ref.sum(1)
    lim = bar.sum(1) + 2.0 ** -24 * want.abs()
    assert bool(((out["seq"].double() - want).abs() <= lim).all()), (out["seq"], want, lim)
    n = int(valid.sum())
    if n == 0:
        assert math.isnan(out["loss"])
        return
    want_loss = -float(ref.sum()) / n
    assert abs(out["loss"] - want_loss) <= float(bar.sum()) / n + 2.0 ** -24 * abs(want_loss), (out["loss"], want_loss)


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 3), (1, 4), (1, 5), (3, 43), (1, 257)]  # rows: below, at and above the 4 of a workgroup; 65 workgroups
WIDTHS = [1, 2, 63, 64, 65, 81, 129, 1000]                    # columns: one lane, around the wave's 64, the vocabulary, 16 per lane


@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("V", WIDTHS)
def test_op_against_float64(gu, V, pad):
    g = torch.Generator().manual_seed(1000 * V + pad)
    worst, worst_e = 0.0, 0.0
    for B, S in SHAPES:
        M = B * S
        x = torch.randn((M, V), generator=g) * 8.0
        t = torch.randint(0, V, (M,), generator=g)
        t[0] = V - 1
        if M >= 3:
            t[2] = 0
            t[1::5] = IGNORE
        if B == 3:
            t[S:2 * S] = IGNORE  # an all-ignored sequence between two valid ones
        out = score_op(gu, padded(x, V + pad), V, B, S, t)
        ref, e_torch, own = reference(x, t)
        r, bar = check_tokens(out["lp"], ref, e_torch, own)
        assert bool((out["lp"].flatten()[t == IGNORE] == 0).all())
        check_sums(out, ref, bar, t, B, S)
        worst, worst_e = max(worst, r), max(worst_e, e_torch)
        # targets = NULL: the row's argmax, and its log-probability
        arg = score_op(gu, padded(x, V + pad), V, B, S, None, chosen=True)
        best = x.argmax(-1)
        assert arg["chosen"].flatten().tolist() == best.tolist()
        ref_a, e_a, own_a = reference(x, best)
        r_a, bar_a = check_tokens(arg["lp"], ref_a, e_a, own_a)
        check_sums(arg, ref_a, bar_a, best, B, S)
        worst = max(worst, r_a)
        # the same rows, the same bits whichever way the target came
        same = t == best
        assert torch.equal(out["lp"].flatten()[same], arg["lp"].flatten()[same])
    record_figure("decoder_score_op", V=V, ld=V + pad, worst_error_over_bar=worst, e_torch=worst_e)
    print(f"decoder_score_op V={V} ld={V + pad}: worst error / bar {worst:.3f} (e_torch {worst_e:.3e})")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("V", WIDTHS[1:])
def test_op_handmade_rows(gu, V, pad):
    g = torch.Generator().manual_seed(77 + V)
    inf = float("inf")
    rnd = lambda: torch.randn((V,), generator=g) * 8.0  # noqa: E731
    big = torch.full((V,), -80.0)
    big[V - 1] = 80.0
    hole = rnd()
    hole[0] = -inf
    rows = [torch.full((V,), 3.25), big, big.clone(),   # sequence 0: all equal; one entry +80, scored at it and away from it
            hole, rnd(), rnd(),                         # sequence 1: a -inf entry; an ignored row; target 0
            rnd(), rnd(), rnd()]                        # sequence 2: all ignored
    t = [0, V - 1, 0, V - 1, IGNORE, 0, IGNORE, IGNORE, IGNORE]
    x = torch.stack(rows)
    out = score_op(gu, padded(x, V + pad), V, 3, 3, t)
    ref, e_torch, own = reference(x, t)
    assert bool(torch.isfinite(ref).all()) and abs(float(ref[0]) + math.log(V)) < 1e-12 and float(ref[2]) < -159.0
    r, bar = check_tokens(out["lp"], ref, e_torch, own)
    assert r <= 1.0, r
    assert out["lp"].flatten()[[4, 6, 7, 8]].tolist() == [0.0] * 4 and out["cnt"].tolist() == [3, 2, 0] and float(out["seq"][2]) == 0.0
    check_sums(out, ref, bar, t, 3, 3)
    want = F.cross_entropy(x.double(), torch.as_tensor(t))  # torch's own mean over the labels that count
    assert abs(out["loss"] - float(want)) <= float(bar.sum()) / 5 + 2.0 ** -24 * abs(float(want))
    # a fourth sequence of rows without a finite answer: all -inf, a +inf entry, a NaN entry; then labels that are no index
    ninf, pinf, nan = torch.full((V,), -inf), rnd(), rnd()
    pinf[V - 1], nan[0] = inf, float("nan")
    x4 = torch.cat([x, torch.stack([ninf, pinf, nan])])
    t4 = t + [0, 0, V - 1]
    out4 = score_op(gu, padded(x4, V + pad), V, 4, 3, t4)
    ref4, e4, own4 = reference(x4, t4)
    assert torch.isnan(own4).tolist() == [False] * 9 + [True] * 3
    check_tokens(out4["lp"], ref4, e4, own4)
    assert torch.equal(out4["lp"][:3], out["lp"]) and torch.equal(out4["seq"][:3], out["seq"]) and out4["cnt"].tolist() == [3, 2, 0, 3]
    assert math.isnan(float(out4["seq"][3])) and math.isnan(out4["loss"])
    assert math.isnan(float(F.cross_entropy(x4, torch.as_tensor(t4))))
    t5 = t + [V, -1, 2 ** 30]  # never used as an index: NaN, and counted, so the loss says so
    out5 = score_op(gu, padded(torch.cat([x, x[3:6]]), V + pad), V, 4, 3, t5)
    assert bool(torch.isnan(out5["lp"][3]).all()) and out5["cnt"].tolist() == [3, 2, 0, 3] and math.isnan(out5["loss"])
    assert torch.equal(out5["lp"][:3], out["lp"])
    # every label ignored: 0 tokens, the mean over none is NaN as torch's is
    none = score_op(gu, padded(x[:6], V + pad), V, 2, 3, [IGNORE] * 6)
    assert none["lp"].flatten().tolist() == [0.0] * 6 and none["cnt"].tolist() == [0, 0] and none["seq"].tolist() == [0.0, 0.0]
    assert math.isnan(none["loss"]) and math.isnan(float(F.cross_entropy(x[:6], torch.full((6,), IGNORE))))
    # targets = NULL: an exact tie goes to the lower index, the first NaN wins, an all -inf row chooses index 0
    tie = rnd().clamp(max=20.0)
    tie[0] = tie[V - 1] = 31.5
    tie2 = tie.clone()
    tie2[0] = 31.0
    tie2[V // 2] = 31.5
    two_nan = rnd()
    two_nan[V // 2] = two_nan[V - 1] = float("nan")
    xa = torch.stack([tie, tie2, two_nan, ninf, pinf])
    arg = score_op(gu, padded(xa, V + pad), V, 1, 5, None, chosen=True)
    assert arg["chosen"].flatten().tolist() == [0, V // 2, V // 2, 0, V - 1]
    assert arg["chosen"].flatten().tolist() == xa.argmax(-1).tolist()  # torch's rule
    ref_a, e_a, own_a = reference(xa[:2], [0, V // 2])
    r_a, _ = check_tokens(arg["lp"].flatten()[:2], ref_a, e_a, own_a)
    assert r_a <= 1.0 and bool(torch.isnan(arg["lp"].flatten()[2:]).all())


def test_op_single_column(gu):
    x = torch.tensor([[3.0], [-1e30], [float("-inf")], [7.0]])
    out = score_op(gu, padded(x, 8), 1, 2, 2, [0, 0, 0, IGNORE])
    assert out["lp"].flatten()[:2].tolist() == [0.0, 0.0] and math.isnan(float(out["lp"][1, 0])) and float(out["lp"][1, 1]) == 0.0
    assert out["cnt"].tolist() == [2, 1] and float(out["seq"][0]) == 0.0


# ---- 2. row independence ----------------------------------------------------------------------------------------------------------
def test_row_independence_bitwise(gu):
    g = torch.Generator().manual_seed(5)
    row = torch.randn((81,), generator=g) * 8.0
    target = 17
    got = []
    for M, at in ((1, 0), (5, 2), (257, 256)):
        for ld in (81, 88):
            x = torch.randn((M, 81), generator=g) * (3.0 + M)  # other neighbours every time
            x[at] = row
            t = torch.randint(0, 81, (M,), generator=g)
            t[at] = target
            given = score_op(gu, padded(x, ld), 81, 1, M, t, reduce=False)["lp"][0, at]
            arg = score_op(gu, padded(x, ld), 81, M, 1, None, chosen=True, reduce=False)
            assert int(arg["chosen"][at, 0]) == int(row.argmax())
            got.append((given.view(torch.int32).item(), arg["lp"][at, 0].view(torch.int32).item()))
    assert len(set(got)) == 1, got
    ref, e_torch, own = reference(row[None], [target])
    assert check_tokens(torch.tensor([got[0][0]], dtype=torch.int32).view(torch.float32), ref, e_torch, own)[0] <= 1.0


# ---- 3. forward(labels=) against the float64 oracle -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g13_seed():
    return int(golden("g13_decoder.npz")["decoder_seed"])


_sds = {}


def decoder_sd(gu, seed):
    if seed not in _sds:
        _sds[seed] = gu.la.synth.decoder_state_dict(seed)
    return _sds[seed]


def labels_for(gu, B, S):
    """Labels of the sweep's ids (label t = id t + 1, the last one </s>), then -100 over a row's tail, inside a row, over a whole row."""
    ids = torch.from_numpy(cases.teacher_forced_ids(gu.la.synth, B, S))
    labels = torch.cat([ids[:, 1:], torch.full((B, 1), 2)], dim=1)
    if S >= 3:
        labels[0, S - S // 3:] = IGNORE
        labels[min(1, B - 1), 1 if B > 1 else 0] = IGNORE
    if B >= 2:
        labels[B - 1] = IGNORE
    return labels


def restated_shift(labels):
    ids = torch.full_like(labels, 2)
    ids[:, 1:] = labels[:, :-1]
    return torch.where(ids == IGNORE, torch.ones_like(ids), ids)


@pytest.mark.parametrize("B,S,T,frames", [c for c in cases.TEACHER_FORCED if c[:3] in ((1, 1, 1), (2, 2, 64), (3, 65, 257), (65, 3, 49))],
                         ids=lambda v: str(v) if isinstance(v, int) else "f")
def test_forward_labels_against_oracle(gu, g13_seed, monkeypatch, B, S, T, frames):
    synth = gu.la.synth
    enc = (synth.hashed_uniform(f"dec_oracle/enc/{B}/{S}/{T}", (B, T, 768), 2) * np.float32(1.5)).astype(np.float32)
    labels = labels_for(gu, B, S)
    valid = labels != IGNORE
    if S >= 3:
        assert not bool(valid[0, -1]) and bool(valid[0, 0]) and bool((~valid[:, 1:-1]).any())
    assert B == 1 or not bool(valid[B - 1].any())
    model = full_model(gu, seed=g13_seed)
    device = torch.device("cuda", 0)
    model.speecht5.encoder._ensure_handle(device)
    model.speecht5.encoder._sync_weights(device, 8)
    enc_dev, fr_dev = gu.dev(enc), gu.dev(np.asarray(frames), torch.int32)
    monkeypatch.setattr(model, "_encode", lambda x, m: (enc_dev, fr_dev))  # both sides decode the same fp32 encoder output
    x = torch.zeros((B, 400))
    out = model(x, labels=labels.to("cuda"))
    ids = restated_shift(labels)
    explicit = model(x, decoder_input_ids=ids.to("cuda"), labels=labels)
    plain = model(x, decoder_input_ids=ids.to("cuda"))
    torch.cuda.synchronize()
    assert plain.loss is None and plain.token_logprobs is None
    assert torch.equal(out.logits, plain.logits) and torch.equal(explicit.logits, plain.logits)
    assert torch.equal(out.token_logprobs, explicit.token_logprobs)
    assert out.loss.shape == () and out.loss.is_cuda and out.loss.view(torch.int32).item() == explicit.loss.view(torch.int32).item()
    sc = model.score(x, labels=labels)  # the same path without the logits
    assert torch.equal(sc.token_logprobs, out.token_logprobs) and sc.tokens.tolist() == valid.sum(1).tolist()
    assert sc.loss.view(torch.int32).item() == out.loss.view(torch.int32).item()
    want_logits = dec_oracle.forward(enc, frames, ids.numpy(), decoder_sd(gu, g13_seed), torch.float64)
    logits, lp = out.logits.cpu().double(), out.token_logprobs.cpu().double()
    assert lp.shape == (B, S) and bool((lp[~valid] == 0).all())
    delta = (logits - want_logits).abs().amax(-1)  # [B, S]: log_softmax moves by at most twice the sup-norm change of its input
    ref = torch.log_softmax(want_logits, -1).gather(-1, labels.clamp(min=0)[..., None])[..., 0] * valid
    lim = 2 * delta + floor_of(ref)
    err = (lp - ref).abs()
    n = int(valid.sum())
    ref_loss = -float(ref.sum()) / n
    lim_loss = 2 * float(delta.max()) + float(floor_of(ref_loss))
    record_figure("decoder_score_forward_labels", B=B, S=S, T_enc=T, worst_error_over_bar=float((err / lim).max()), delta_max=float(delta.max()),
                  loss=float(out.loss), loss_ref=ref_loss, loss_error_over_bar=abs(float(out.loss) - ref_loss) / lim_loss)
    print(f"forward(labels) B={B} S={S}: worst token error / bar {float((err / lim).max()):.3f}, loss {float(out.loss):.7f} vs {ref_loss:.7f}")
    assert bool((err <= lim).all()), float((err / lim).max())
    assert abs(float(out.loss) - ref_loss) <= lim_loss
    seq_ref = ref.sum(1)
    assert bool(((sc.sequence_logprob.cpu().double() - seq_ref).abs() <= (lim * valid).sum(1) + 2.0 ** -24 * seq_ref.abs()).all())


# ---- 4. generate with scores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b1_len2", "b7_len3_ragged", "b7_len10_all_end"])
def test_generate_with_scores(gu, name):
    seed, lengths_of, first_index, max_length = cases.GENERATE[name]
    synth = gu.la.synth
    x, m = synth.batch(lengths_of(synth), first_index=first_index)
    x, m = gu.dev(x), gu.dev(m, torch.int32)
    model = full_model(gu, seed=seed)
    plain = model.generate(x, m, max_length=max_length)
    ids_l, steps = model.generate(x, m, max_length=max_length, return_logits=True)
    same = model.generate(x, m, max_length=max_length, output_scores=True)  # without return_dict_in_generate: nothing changes
    bare = model.generate(x, m, max_length=max_length, return_dict_in_generate=True)
    out = model.generate(x, m, max_length=max_length, return_dict_in_generate=True, output_scores=True)
    lengths = model._decoder_runtime.last_lengths.clone()
    torch.cuda.synchronize()
    assert torch.is_tensor(same) and torch.equal(same, plain) and torch.equal(bare.sequences, plain) and bare.scores is None and bare.token_logprobs is None
    assert torch.equal(out.sequences, plain) and torch.equal(ids_l, plain)
    B, S = plain.shape
    assert isinstance(out.scores, tuple) and len(out.scores) == S - 1 and all(torch.equal(out.scores[t], steps[t]) for t in range(S - 1))
    ids, lp = plain.cpu(), out.token_logprobs.cpu()
    assert lp.shape == (B, S - 1) and out.sequence_logprobs.shape == (B,)
    open_ = torch.arange(1, S)[None, :] < lengths[:, None]  # column t + 1 was generated, not padded
    assert bool((ids[:, 1:][~open_] == 1).all()) and bool((lp[~open_] == 0).all())
    worst = 0.0
    for t in range(S - 1):
        rows = open_[:, t]
        if bool(rows.any()):
            ref, e_torch, own = reference(steps[t].cpu()[rows], ids[rows, t + 1])
            worst = max(worst, check_tokens(lp[rows, t], ref, e_torch, own)[0])
    total = lp.double().sum(1)
    assert bool(((out.sequence_logprobs.cpu().double() - total).abs() <= 2.0 ** -24 * total.abs() + 1e-12).all())
    assert bool((lp[open_] <= 0).all())
    record_figure("decoder_score_generate", case=name, B=B, S=S, worst_error_over_bar=worst)
    assert worst <= 1.0, worst
    if name == "b7_len10_all_end":  # rows that end at their first token count that one token
        first = lengths == 2
        assert bool(first.any()) and bool((lp[first][:, 1:] == 0).all())
        assert torch.equal(out.sequence_logprobs.cpu()[first], lp[first][:, 0])


# ---- 5. the pool --------------------------------------------------------------------------------------------------------------------
def decode_scores(dec, model, items, slots):
    pool = dec.DecoderPool(model.speecht5.encoder, slots, max(it.rows for it in items), max(it.cap for it in items), torch.device("cuda", 0),
                           return_logits=True, return_scores=True)
    pool.submit(list(items))
    return {k: (ids, lg.cpu(), sc.cpu()) for k, ids, lg, sc in pool.drain()}


def test_pool_scores_do_not_depend_on_the_neighbours(gu, dec):
    model = small_model(gu)
    clips, caps = pc.oracle_clips(gu.la.synth), pc.ORACLE_CAPS
    items, _, _ = encode(gu, model, clips, caps)
    base = decode_scores(dec, model, items, 2)
    assert sorted(base) == list(range(12))
    for other, what in ((decode_scores(dec, model, items, 5), "5 slots"), (decode_scores(dec, model, items[::-1], 5), "reversed")):
        for k, (ids, lg, sc) in base.items():
            assert torch.equal(ids, other[k][0]) and torch.equal(lg, other[k][1]) and torch.equal(sc, other[k][2]), (what, k)
    for k, (ids, lg, sc) in base.items():  # the kernel on the utterance's own logits: the same bits
        n = len(ids)
        assert sc.shape == (n - 1,) and lg.shape == (n - 1, 81)
        alone = score_op(gu, lg, 81, 1, n - 1, None, chosen=True, reduce=False)
        assert torch.equal(alone["lp"][0], sc), k
        assert alone["chosen"][0].tolist() == ids[1:].tolist()
        assert bool((sc <= 0).all())  # 0: a step whose other logits all lie a float's precision below the chosen one
    # generate_many: the same ids with and without scores, scores that are the kernel's on the logits returned beside them
    batches = batches_of(gu, clips)
    ids0 = model.generate_many(batches, max_length=caps, slots=pc.ORACLE_SLOTS)
    ids1, scores = model.generate_many(batches, max_length=caps, slots=pc.ORACLE_SLOTS, return_scores=True)
    ids2, logits, scores2 = model.generate_many(batches, max_length=caps, slots=5, return_logits=True, return_scores=True)
    assert len(scores) == 12 and all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(ids0, ids1, ids2))
    for u in range(12):
        assert scores[u].is_cuda and scores[u].shape == (len(ids0[u]) - 1,)
        assert torch.equal(scores[u], scores2[u])
        assert torch.equal(score_op(gu, logits[u].cpu(), 81, 1, len(ids0[u]) - 1, None, reduce=False)["lp"][0], scores[u].cpu())


# ---- 6. score_many -------------------------------------------------------------------------------------------------------------------
def test_score_many_against_score_per_pair(gu, dec):
    model = small_model(gu)
    oc = pc.oracle_clips(gu.la.synth)
    clips = oc[0:4] + oc[10:12]  # three reference pairs of unequal lengths, within and between the pairs
    batches = batches_of(gu, clips)
    assert len({int(b["input_values"].shape[1]) for b in batches}) == 3
    g = torch.Generator().manual_seed(3)
    labels = []
    for n in (5, 1, 9, 12, 2, 7):
        row = torch.randint(4, 81, (n,), generator=g)
        row[-1] = 2
        labels.append(row)
    enc = model.speecht5.encoder

    def packed_logits(group, rows):
        """The logits score_many's pass computes for a group of batches: the packed encoder output, the labels padded with -100."""
        ticket = enc.forward_packed_async(group)
        ticket.result()
        out, _ = ticket.packed_output()
        S = max(len(r) for r in rows)
        lab = torch.full((len(rows), S), IGNORE)
        for i, r in enumerate(rows):
            lab[i, :len(r)] = r
        ids = dec.shift_tokens_right(lab).to(device="cuda", dtype=torch.int32)
        return model._decoder_runtime.forward(out, enc.last_frames, ids)[0].cpu().double()

    per_pair, pair_logits = [], []
    for i, b in enumerate(batches):
        rows = labels[2 * i:2 * i + 2]
        lab = torch.full((2, max(len(r) for r in rows)), IGNORE)
        for j, r in enumerate(rows):
            lab[j, :len(r)] = r
        sc = model.score(**b, labels=lab)
        out = model(**b, labels=lab)
        assert torch.equal(sc.token_logprobs, out.token_logprobs)
        for j, r in enumerate(rows):
            per_pair.append(sc.token_logprobs[j, :len(r)].cpu().double())
            pair_logits.append(out.logits[j, :len(r)].cpu().double())
    worst = 0.0
    for pack in (1, 3):
        got = model.score_many(batches, labels, pack=pack)
        assert len(got) == 6
        lg = torch.cat([packed_logits(batches[g0:g0 + pack], labels[2 * g0:2 * (g0 + pack)]) for g0 in range(0, 3, pack)]) if pack == 3 else None
        for u, (lp, total) in enumerate(got):
            assert lp.is_cuda and lp.shape == (len(labels[u]),) and total.shape == ()
            if pack == 3:
                delta = (lg[u, :len(labels[u])] - pair_logits[u]).abs().amax(-1)
            else:
                i = u // 2
                delta = (packed_logits(batches[i:i + 1], labels[2 * i:2 * i + 2])[u % 2, :len(labels[u])] - pair_logits[u]).abs().amax(-1)
            lim = 2 * delta + floor_of(per_pair[u])
            err = (lp.cpu().double() - per_pair[u]).abs()
            worst = max(worst, float((err / lim).max()))
            assert bool((err <= lim).all()), (pack, u, err, lim)
            s = lp.cpu().double().sum()
            assert abs(float(total) - float(s)) <= 2.0 ** -24 * abs(float(s)) + 1e-12
    record_figure("decoder_score_many", worst_error_over_bar=worst)


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------
def test_transcribe_scores(gu, tmp_path, monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = small_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on; 2-layer weights keep it quick
    common = ["--random-init", "--synthetic", "4", "--synthetic-seconds", "1", "--max-length", "6"]
    paths = {k: tmp_path / f"{k}.jsonl" for k in ("loop", "pool", "loop_scores", "pool_scores")}
    assert tr.main(common + ["--out", str(paths["loop"])]) == 0
    assert tr.main(common + ["--slots", "4", "--out", str(paths["pool"])]) == 0
    assert tr.main(common + ["--scores", "--out", str(paths["loop_scores"])]) == 0
    assert tr.main(common + ["--scores", "--slots", "4", "--out", str(paths["pool_scores"])]) == 0
    plain = [json.loads(l) for l in paths["loop"].read_text().splitlines()]
    assert len(plain) == 4 and all(sorted(r) == ["id", "token_ids"] for r in plain)
    assert paths["pool"].read_text() == paths["loop"].read_text()
    for k in ("loop_scores", "pool_scores"):
        recs = [json.loads(l) for l in paths[k].read_text().splitlines()]
        assert len(recs) == 4
        for r, p in zip(recs, plain):
            assert sorted(r) == ["avg_logprob", "id", "logprob", "token_ids"]
            assert r["id"] == p["id"] and r["token_ids"] == p["token_ids"]  # without the flag: the same fields, the same values
            row = r["token_ids"]
            tokens = row.index(2, 1) + 1 if 2 in row[1:] else len(row)  # <s> ... up to and including </s>; <pad> after it is not generated
            assert math.isfinite(r["logprob"]) and r["logprob"] <= 0
            assert r["avg_logprob"] == r["logprob"] / (tokens - 1), (k, r)
