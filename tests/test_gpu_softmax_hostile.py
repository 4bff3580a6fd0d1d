"""-m gpu: the online softmaxes that had no input taking their rescale branch late -- dec_attention_kernel + dec_attention_combine,
dec_attention_probs and the intent head's attention pooling across its 128-frame splits -- on inputs whose running maximum jumps in the
last tile, at a split's first key, at keys 63 / 64, in every tile, or never (value_domain_cases.py builds them, test_value_domain_ref.py
checks that they do what they say and that torch's own fp32 evaluation stays well inside the fixed bars).

The reference is float64 throughout.  Per output row the bar is max(4 x the largest error of torch's CPU fp32 evaluation of that row
against float64, 2^-21 max(1, |ref|)) -- the rule of tests/test_gpu_decoder_score.py -- and the project's whole-tensor bars are asserted
beside it: 1e-5 relative L2 for the attention output (test_gpu_decoder.BAR_ATTN), 1e-5 max abs for probabilities
(test_gpu_decoder_attn.TOL), 2e-5 for the head's logits, loss, dW and db and 1e-5 for its dq (test_gpu_intent_head.py)."""
import numpy as np
import pytest
import torch

import intent_head_oracle as iho
import value_domain_cases as vd
from conftest import record_figure

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpu_util import check, dev, la, lib, ptr, rel_l2, stream

BAR_ATTN = 1e-5
BAR_PROBS = 1e-5
BAR_HEAD, BAR_HEAD_DQ = 2e-5, 1e-5


# ---- loco_op_decoder_attention ----------------------------------------------------------------------------------------------------------
def attention_op(q, k, v, causal, offset):
    """Two launches on the same buffers; the second must reproduce the first bit for bit (fixed-order combine)."""
    B, Sq, Tk = q.shape[0], q.shape[1], k.shape[1]
    nb = int(lib().loco_decoder_attention_scratch_bytes(B, Sq, Tk))
    scratch = torch.empty(max(nb, 4), dtype=torch.uint8, device="cuda")
    qd, kd, vd_ = dev(q), dev(k), dev(v)
    outs = []
    for _ in range(2):
        out = torch.full((B, Sq, 768), float("nan"), device="cuda")
        check(lib().loco_op_decoder_attention(ptr(qd), ptr(kd), ptr(vd_), None, ptr(out), B, Sq, Tk, causal, offset, vd.SCALE, ptr(scratch), scratch.numel(),
                                              stream()), "decoder_attention")
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    return outs[0].cpu(), nb


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("Tk", [600, 200])  # 600: three key splits of 256, the smallest shape with a middle split; 200: one split
@pytest.mark.parametrize("kind", vd.ATTN_KINDS)
def test_decoder_attention_hostile_scores(kind, Tk, Sq, causal):
    q, k, v = vd.decoder_attention_case(kind, Sq, Tk)
    offset = Tk - Sq if causal else 0
    ref = vd.attention_ref(q, k, v, None, causal, offset)
    own = vd.attention_ref(q, k, v, None, causal, offset, torch.float32)
    out, nb = attention_op(q, k, v, causal, offset)
    assert (nb > 0) == (Tk == 600)
    assert bool(torch.isfinite(out).all())
    bar = vd.row_bar(ref, own)
    fig = dict(rel_l2=rel_l2(out, ref), over_row_bar=vd.worst_ratio(out, ref, bar), max_abs=float((out.double() - ref).abs().max()),
               torch_fp32_max_abs=float((own.double() - ref).abs().max()))
    record_figure("decoder_attention_hostile", kind=kind, Tk=Tk, Sq=Sq, causal=causal, **fig)
    print("decoder attention", kind, Tk, Sq, causal, fig)
    assert fig["over_row_bar"] <= 1.0, fig
    assert fig["rel_l2"] <= BAR_ATTN, fig


# ---- loco_op_decoder_attention_probs ----------------------------------------------------------------------------------------------------
def probs_op(q, k, counts, causal):
    B, Sq, Tk = q.shape[0], q.shape[1], k.shape[1]
    qd, kd = dev(q), dev(k)
    kc = dev(np.asarray(counts), torch.int32) if counts is not None else None
    P = torch.full((B, 12, Sq, Tk), -7.0, device="cuda")
    check(lib().loco_op_decoder_attention_probs(ptr(qd), ptr(kd), ptr(kc), ptr(P), B, Sq, Tk, int(causal), 768, Sq * 768, 768, Tk * 768, vd.SCALE, stream()),
          "decoder_attention_probs")
    torch.cuda.synchronize()
    return P.cpu()


@pytest.mark.parametrize("Tk", [65, 257])
@pytest.mark.parametrize("kind", vd.PROBS_KINDS)
def test_decoder_attention_probs_hostile_scores(kind, Tk):
    """Key counts [Tk, Tk - 3] (the second clip never sees the leading key), then the causal form on a square launch."""
    worst = {}
    for name, B, Sq, counts, causal in (("counts", 2, 3, [Tk, Tk - 3], False), ("causal", 1, Tk, None, True)):
        q, k = vd.decoder_probs_case(kind, B, Sq, Tk)
        ref, vis = vd.probs_ref(q, k, counts, causal)
        own, _ = vd.probs_ref(q, k, counts, causal, torch.float32)
        P = probs_op(q, k, counts, causal)
        assert bool(torch.isfinite(P).all()) and bool((P[~vis] == 0).all())  # masked entries: exactly 0
        bar = vd.row_bar(ref, own)
        row_sum_bar = bar.sum(-1)   # a row's sum is held to the sum of its elements' bars
        worst[name + "_over_row_bar"] = vd.worst_ratio(P, ref, bar)
        worst[name + "_max_abs"] = float((P.double() - ref).abs().max())
        worst[name + "_row_sum"] = float((P.double().sum(-1) - 1).abs().max())
        worst[name + "_row_sum_over_bar"] = float(((P.double().sum(-1) - 1).abs() / row_sum_bar).max())
    record_figure("decoder_attention_probs_hostile", kind=kind, Tk=Tk, **worst)
    print("decoder attention probabilities", kind, Tk, worst)
    for name in ("counts", "causal"):
        assert worst[name + "_over_row_bar"] <= 1.0 and worst[name + "_row_sum_over_bar"] <= 1.0, worst
        assert worst[name + "_max_abs"] <= BAR_PROBS and worst[name + "_row_sum"] <= BAR_PROBS, worst


# ---- the intent head's attention pooling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [300, 129])  # splits of 128 / 128 / 44, and 128 / 1
def test_intent_head_attention_pooling_hostile_scores(T):
    q = vd.head_query()
    W, b = vd.head_params()
    x, target = vd.head_batch(T, q)
    ref = vd.head_reference(iho.IntentClassifierOracle, q, W, b, x, target, torch.float64)
    own = vd.head_reference(iho.IntentClassifierOracle, q, W, b, x, target, torch.float32)
    head = la.IntentClassifierMI355X("attention")
    head.load_state_dict({"q": q[None].clone(), "classifier.0.weight": W.clone(), "classifier.0.bias": b.clone()})
    head = head.to("cuda")
    logits = head(x.cuda())
    assert tuple(logits.shape) == (3, 1, 101)
    loss, _, grads = head.loss_and_grads(x.cuda(), target.cuda())
    torch.cuda.synchronize()
    g = grads.cpu()
    got = dict(logits=logits.cpu().squeeze(1), loss=loss.detach().cpu().reshape(1), dW=g[768:768 + 101 * 768].view(101, 768), db=g[768 + 101 * 768:][None],
               dq=g[:768][None])
    fig = {}
    for name in ("logits", "loss", "dW", "db", "dq"):
        assert bool(torch.isfinite(got[name]).all()), name
        fig[name] = rel_l2(got[name], ref[name])
        fig[name + "_torch_fp32"] = rel_l2(own[name], ref[name])
        fig[name + "_over_row_bar"] = vd.worst_ratio(got[name], ref[name], vd.row_bar(ref[name], own[name]))
    record_figure("intent_head_attention_hostile", T=T, **fig)
    print("intent head, attention pooling, T =", T, fig)
    for name in ("logits", "loss", "dW", "db", "dq"):
        assert fig[name + "_over_row_bar"] <= 1.0, (name, fig)
        assert fig[name] <= (BAR_HEAD_DQ if name == "dq" else BAR_HEAD), (name, fig)
