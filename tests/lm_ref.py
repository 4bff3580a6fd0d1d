"""float64 restatement of what loco-asr_amd/lm.py computes: GPT-2 (HF GPT2LMHeadModel, pre-LN, gelu_new, tied head), the token NLL and
the reference's two corpus walkers.  numpy only; the checker, never the product.  Written from the model's definition, not from lm.py."""
import math
import re
from collections import OrderedDict

import numpy as np

HIDDEN, HEADS, HEAD_DIM = 768, 12, 64


def _get(sd, key):
    v = sd[key] if key in sd else sd["transformer." + key]
    return np.asarray(v, np.float64)


def layernorm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def gelu_new(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def n_layers(sd):
    return 1 + max(int(m.group(1)) for m in (re.search(r"(?:^|\.)h\.(\d+)\.ln_1\.weight$", k) for k in sd) if m)


def hidden_states(sd, ids, mask=None):
    """ids: 1-D int sequence (one sequence; causal attention makes right padding irrelevant to the valid positions).  Returns the
    n_layer + 1 hidden states HF reports ([S, 768] each: embedding output, blocks 0 .. n - 2, ln_f of the last block).
    mask (optional, bool [S, S], every layer and head): entry (t, j) says whether query t sees key j, in place of the causal rule j <= t
    -- for tests that plant an attention fault in this reference to see how far the NLLs move."""
    ids = np.asarray(ids, np.int64)
    S = len(ids)
    x = _get(sd, "wte.weight")[ids] + _get(sd, "wpe.weight")[:S]
    out = [x]
    L = n_layers(sd)
    mask = np.tril(np.ones((S, S), bool)) if mask is None else np.asarray(mask, bool).reshape(S, S)
    for l in range(L):
        p = f"h.{l}."
        h = layernorm(x, _get(sd, p + "ln_1.weight"), _get(sd, p + "ln_1.bias"))
        qkv = h @ _get(sd, p + "attn.c_attn.weight") + _get(sd, p + "attn.c_attn.bias")
        q, k, v = (qkv[:, i * HIDDEN:(i + 1) * HIDDEN].reshape(S, HEADS, HEAD_DIM).transpose(1, 0, 2) for i in range(3))
        sc = q @ k.transpose(0, 2, 1) / 8.0
        sc = np.where(mask[None], sc, -np.inf)
        sc = sc - sc.max(-1, keepdims=True)
        pr = np.exp(sc)
        pr /= pr.sum(-1, keepdims=True)
        ctx = (pr @ v).transpose(1, 0, 2).reshape(S, HIDDEN)
        x = x + ctx @ _get(sd, p + "attn.c_proj.weight") + _get(sd, p + "attn.c_proj.bias")
        h = layernorm(x, _get(sd, p + "ln_2.weight"), _get(sd, p + "ln_2.bias"))
        h = gelu_new(h @ _get(sd, p + "mlp.c_fc.weight") + _get(sd, p + "mlp.c_fc.bias"))
        x = x + h @ _get(sd, p + "mlp.c_proj.weight") + _get(sd, p + "mlp.c_proj.bias")
        if l + 1 < L:
            out.append(x)
    out.append(layernorm(x, _get(sd, "ln_f.weight"), _get(sd, "ln_f.bias")))
    return out


def head_nll(h, wte, targets, ignore_index=-100):
    """nll[r] = logsumexp_v(h[r] . wte[v]) - h[r] . wte[t[r]] in float64; 0 for ignore_index, NaN for another target outside [0, V)."""
    h, wte = np.asarray(h, np.float64), np.asarray(wte, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        z = h @ wte.T
        m = z.max(-1, keepdims=True)
        lse = (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))[:, 0]
    out = np.empty(len(h))
    for r, t in enumerate(np.asarray(targets)):
        out[r] = 0.0 if t == ignore_index else (np.nan if t < 0 or t >= len(wte) else lse[r] - z[r, t])
    return out


def token_nll(sd, ids, mask=None):
    """[S - 1] float64: entry s = -log P(ids[s + 1] | ids[:s + 1]).  mask: see hidden_states."""
    h = hidden_states(sd, ids, mask)[-1]
    return head_nll(h[:-1], _get(sd, "wte.weight"), np.asarray(ids)[1:])


# ---- the two context modes, restated -------------------------------------------------------------------------------------------
def indep_batches(lines, tok, bsize):
    """lines: [(utt_id, text)].  Returns (utt_ids in scoring order, [batch = list of id lists])."""
    seen, ids, keys = set(), [], []
    for utt_id, text in lines:
        if utt_id in seen:
            continue
        seen.add(utt_id)
        ids.append([tok.bos_token_id] + list(tok(text)["input_ids"]) + [tok.eos_token_id])
        keys.append(utt_id)
    lengths = np.asarray([len(t) for t in ids])
    order = np.argsort(lengths)
    ids, keys = [ids[i] for i in order], [keys[i] for i in order]
    batches = []
    for n in sorted(set(lengths.tolist())):
        same = [t for t in ids if len(t) == n]
        batches += [same[i:i + bsize] for i in range(0, len(same), bsize)]
    return keys, batches


def max_len_batches(lines, tok, max_len, bsize):
    """[(batch = list of id lists, rec_ids, first, last)] in the reference's order, with its two quirks."""
    seen = OrderedDict()
    for utt_id, text in lines:
        seen.setdefault(utt_id, text)

    def key(u):
        rec, _, a, b = u.split("-")
        return "-".join((rec, a, b))

    recs = OrderedDict()
    for u in sorted(seen, key=key):
        recs.setdefault(u.split("-", 1)[0], []).extend(list(tok(seen[u])["input_ids"]) + [tok.eos_token_id])
    out = []
    for rec, v in recs.items():
        if len(v) < max_len:
            out.append(([v], [rec], True, True))
            continue
        wins = [v[o:o + max_len] for o in range(len(v) - max_len)]  # never the window that ends at the final token
        if not wins:
            continue  # exactly max_len tokens: nothing
        out.append(([wins[0]], [rec], True, len(wins) == 1))
        rest = wins[1:]
        for i in range(0, len(rest), bsize):
            out.append((rest[i:i + bsize], [rec] * len(rest[i:i + bsize]), False, i + bsize >= len(rest)))
    return out


def fold(nlls, ids):
    """The reference's compute_ppl_per_recording, in float64."""
    rec = OrderedDict()
    for v, u in zip(nlls, ids):
        rec.setdefault(u.split("-", 1)[0], []).extend(v)
    return rec, {r: float(np.exp(np.mean(np.asarray(v, np.float64)))) for r, v in rec.items()}
