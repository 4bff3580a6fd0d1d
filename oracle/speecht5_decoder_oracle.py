"""CPU oracle for the SpeechT5 text decoder (teacher-forced logits and greedy search).  TEST INFRASTRUCTURE ONLY.

Like ``speecht5_oracle.py`` this file is the checker, never the product: only ``tests/`` and ``tools/`` import it, and it imports
nothing from the package under test.  It restates, in plain torch CPU ops and any dtype, what HuggingFace's
``SpeechT5ForSpeechToText`` does after the encoder (``HF:`` = ``transformers/models/speecht5/modeling_speecht5.py`` 5.15.0):

  SpeechT5TextDecoderPrenet   HF:782-816   embed_tokens[ids] * 1 (scale_embedding is False) + sinusoid[position ids]
  position ids                HF:337-351   (cumsum(ids != <pad>) + past length) * (ids != <pad>) + padding_idx, padding_idx = 1
  SpeechT5Attention           HF:872-986   q, k, v separate projections, q * head_dim**-0.5, additive mask, softmax, out_proj
  SpeechT5DecoderLayer        HF:1095-1158 post-LN: self-attention, cross-attention, feed-forward, each residual + LayerNorm
  SpeechT5Decoder             HF:1449-1590 causal mask only (no decoder padding mask: <pad> tokens are keys like any other);
                                           encoder keys at and beyond a clip's frame count are masked
  SpeechT5TextDecoderPostnet  HF:819-826   lm_head, no bias

Weights come as the numpy dict ``synth.decoder_state_dict(seed)`` returns (HF's names below ``speecht5.`` and
``text_decoder_postnet.lm_head.weight``).  Masks are additive ``-inf`` (HF adds ``finfo.min``: the same softmax wherever a row
keeps one visible key, which every row here does).  No fusion, and no cache beyond the k/v cache of ``greedy``.

Pinned to HF by ``tests/test_decoder_oracle.py`` (fixture g13: HF in fp32 and float64) and, where ``transformers`` is importable,
by ``tests/test_decoder_oracle_vs_hf.py`` (HF's own modules at other shapes).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from speecht5_oracle import HEADS, LN_EPS, _t, gelu_erf, sinusoid_table

PAD = 1    # SpeechT5Config.pad_token_id = padding_idx of the position table
EOS = 2    # eos_token_id = decoder_start_token_id
MAX_TEXT_POSITIONS = 450
DEC = "decoder.wrapped_decoder.layers."


def num_layers(sd):
    n = 0
    while f"{DEC}{n}.final_layer_norm.weight" in sd:
        n += 1
    return n


def cast_weights(sd, dtype):
    """Every tensor of ``sd`` as a torch tensor of ``dtype``, once per call of ``forward`` / ``greedy`` (not once per step)."""
    return {k: _t(sd, k, dtype) for k in sd}


def position_ids(ids, past=0):
    """HF:337-351.  <pad> -> 1 (the zero row); the n-th non-pad token of a row -> n + 1 + past."""
    mask = ids.ne(PAD).int()
    return ((torch.cumsum(mask, dim=1).type_as(mask) + past) * mask).long() + PAD


def prenet(ids, sd, dtype, past=0):
    """HF:797-816.  The table has max_text_positions + pad + 1 + offset(2) rows, is built in fp32 and cast (HF:288-320)."""
    tab = sinusoid_table(MAX_TEXT_POSITIONS + PAD + 1 + 2, 768, dtype)
    return _t(sd, "decoder.prenet.embed_tokens.weight", dtype)[ids] + tab[position_ids(ids, past)]


def _heads(x):
    B, S, D = x.shape
    return x.view(B, S, HEADS, D // HEADS).transpose(1, 2)  # [B,H,S,dh]


def project_kv(x, sd, ap, dtype):
    """k_proj / v_proj of ``x`` split into heads (HF:911-914)."""
    k = F.linear(x, _t(sd, ap + "k_proj.weight", dtype), _t(sd, ap + "k_proj.bias", dtype))
    v = F.linear(x, _t(sd, ap + "v_proj.weight", dtype), _t(sd, ap + "v_proj.bias", dtype))
    return _heads(k), _heads(v)


def attend(x, k, v, mask, sd, ap, dtype):
    """HF:891,923-984 for queries x [B,S,768] and keys / values [B,H,Tk,dh]; mask additive, broadcastable to [B,1,S,Tk], or None."""
    B, S, D = x.shape
    q = F.linear(x, _t(sd, ap + "q_proj.weight", dtype), _t(sd, ap + "q_proj.bias", dtype)) * (D // HEADS) ** -0.5
    s = _heads(q) @ k.transpose(-1, -2)
    if mask is not None:
        s = s + mask
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, S, D)
    return F.linear(o, _t(sd, ap + "out_proj.weight", dtype), _t(sd, ap + "out_proj.bias", dtype))


def _ln(x, sd, name, dtype):
    return F.layer_norm(x, (x.shape[-1],), _t(sd, name + ".weight", dtype), _t(sd, name + ".bias", dtype), LN_EPS)


def decoder_layer(x, self_k, self_v, self_mask, cross_k, cross_v, cross_mask, sd, lp, dtype):
    """HF:1120-1151."""
    h = _ln(x + attend(x, self_k, self_v, self_mask, sd, lp + "self_attn.", dtype), sd, lp + "self_attn_layer_norm", dtype)
    h = _ln(h + attend(h, cross_k, cross_v, cross_mask, sd, lp + "encoder_attn.", dtype), sd, lp + "encoder_attn_layer_norm", dtype)
    f = gelu_erf(F.linear(h, _t(sd, lp + "feed_forward.intermediate_dense.weight", dtype), _t(sd, lp + "feed_forward.intermediate_dense.bias", dtype)))
    f = F.linear(f, _t(sd, lp + "feed_forward.output_dense.weight", dtype), _t(sd, lp + "feed_forward.output_dense.bias", dtype))
    return _ln(h + f, sd, lp + "final_layer_norm", dtype)


def encoder_key_mask(frames, T, dtype):
    """[B,1,1,T] additive mask: -inf at the encoder rows at and beyond frames[b]; None = every row is a key."""
    if frames is None:
        return None
    frames = torch.as_tensor(frames).long()
    masked = torch.arange(T)[None, :] >= frames[:, None]
    return torch.zeros(masked.shape, dtype=dtype).masked_fill(masked, float("-inf"))[:, None, None, :]


@torch.no_grad()
def forward(enc_out, frames, ids, sd, dtype=torch.float64, hidden_states=None):
    """Teacher-forced pass: enc_out [B,T,768], frames [B] or None, ids [B,S] -> logits [B,S,V]; ``hidden_states`` (a list) is
    filled with the prenet output and every layer's output, 7 tensors [B,S,768] (HF:1546-1575)."""
    sd = cast_weights(sd, dtype)
    enc = torch.as_tensor(enc_out).to(dtype)
    ids = torch.as_tensor(ids).long()
    S = ids.shape[1]
    causal = torch.full((S, S), float("-inf"), dtype=dtype).triu(1)
    cross_mask = encoder_key_mask(frames, enc.shape[1], dtype)
    h = prenet(ids, sd, dtype)
    for l in range(num_layers(sd)):
        if hidden_states is not None:
            hidden_states.append(h)
        lp = f"{DEC}{l}."
        sk, sv = project_kv(h, sd, lp + "self_attn.", dtype)
        ck, cv = project_kv(enc, sd, lp + "encoder_attn.", dtype)
        h = decoder_layer(h, sk, sv, causal, ck, cv, cross_mask, sd, lp, dtype)
    if hidden_states is not None:
        hidden_states.append(h)
    return F.linear(h, _t(sd, "text_decoder_postnet.lm_head.weight", dtype))


@torch.no_grad()
def greedy(enc_out, frames, sd, max_length, dtype=torch.float64):
    """Greedy search as HF's ``generate(do_sample=False, num_beams=1)`` runs it, one token per step on a k/v cache: every row starts
    with </s> (decoder_start_token_id); a row that has emitted </s> takes <pad> from then on; the loop stops after the step in which
    the last open row finishes, or at ``max_length`` tokens.  A step's single token sits at past length t, so a non-pad token gets
    position t + 2 and <pad> position 1 (HF:809-810).

    Returns (ids [B,S] long, step logits [S-1,B,V], lengths [B] = tokens of a row up to and including its </s>, gaps [S-1,B]).
    gaps[t, b] = (best - second-best logit of row b) / max |logit| of step t over all rows: the measure fixture g13 asserts
    >= 1e-3 on (its condition (i)); below that a correct fp32 implementation may pick the other token."""
    sd = cast_weights(sd, dtype)
    enc = torch.as_tensor(enc_out).to(dtype)
    B = enc.shape[0]
    L = num_layers(sd)
    cross_mask = encoder_key_mask(frames, enc.shape[1], dtype)
    cross = [project_kv(enc, sd, f"{DEC}{l}.encoder_attn.", dtype) for l in range(L)]
    cache = [None] * L
    ids = torch.full((B, 1), EOS, dtype=torch.long)
    open_rows = torch.ones(B, dtype=torch.bool)
    lengths = torch.ones(B, dtype=torch.long)
    steps, gaps = [], []
    for t in range(max_length - 1):
        h = prenet(ids[:, -1:], sd, dtype, past=t)
        for l in range(L):
            lp = f"{DEC}{l}."
            k, v = project_kv(h, sd, lp + "self_attn.", dtype)
            if cache[l] is not None:
                k, v = torch.cat([cache[l][0], k], dim=2), torch.cat([cache[l][1], v], dim=2)
            cache[l] = (k, v)
            h = decoder_layer(h, k, v, None, cross[l][0], cross[l][1], cross_mask, sd, lp, dtype)
        logits = F.linear(h[:, 0], _t(sd, "text_decoder_postnet.lm_head.weight", dtype))
        top2 = logits.topk(2, dim=-1).values
        steps.append(logits)
        gaps.append((top2[:, 0] - top2[:, 1]) / logits.abs().max())
        nxt = torch.where(open_rows, logits.argmax(-1), torch.full((B,), PAD))
        ids = torch.cat([ids, nxt[:, None]], dim=1)
        lengths += open_rows.long()
        open_rows = open_rows & nxt.ne(EOS)
        if not bool(open_rows.any()):
            break
    return ids, torch.stack(steps), lengths, torch.stack(gaps)
