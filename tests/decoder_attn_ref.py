"""Float64 references for the decoder's attention probabilities and token alignment (tests only; no GPU, no library import).

``forward_with_attentions`` restates oracle/speecht5_decoder_oracle.py's teacher-forced pass with the probabilities kept: per layer
P_self [B,12,S,S] and P_cross [B,12,S,T], the layer's output formed from P @ v (tests/test_decoder_attn_ref.py pins it to the oracle's
own ``forward`` and, where transformers imports, to HF's ``decoder_attentions`` / ``cross_attentions``).  ``mean_attention`` is the
alignment matrix A, ``dtw`` the monotone path with the tie rule of include/loco_asr.h (diagonal, then (s-1,t), then (s,t-1))."""
import numpy as np
import torch
import torch.nn.functional as F

import speecht5_decoder_oracle as dec_oracle
from speecht5_decoder_oracle import DEC, _heads, _ln, encoder_key_mask, num_layers, prenet, project_kv
from speecht5_oracle import HEADS, _t, gelu_erf


def _attend(x, k, v, mask, sd, ap, dtype):
    """oracle.attend with the probabilities handed out: (out_proj(P @ v), P [B,H,S,Tk])."""
    B, S, D = x.shape
    q = F.linear(x, _t(sd, ap + "q_proj.weight", dtype), _t(sd, ap + "q_proj.bias", dtype)) * (D // HEADS) ** -0.5
    s = _heads(q) @ k.transpose(-1, -2)
    if mask is not None:
        s = s + mask
    P = torch.softmax(s, dim=-1)
    o = (P @ v).transpose(1, 2).reshape(B, S, D)
    return F.linear(o, _t(sd, ap + "out_proj.weight", dtype), _t(sd, ap + "out_proj.bias", dtype)), P


@torch.no_grad()
def forward_with_attentions(enc_out, frames, ids, sd, dtype=torch.float64):
    """(logits [B,S,V], [P_self per layer], [P_cross per layer]); masked entries are exactly 0 (softmax of -inf)."""
    sd = dec_oracle.cast_weights(sd, dtype)
    enc = torch.as_tensor(enc_out).to(dtype)
    ids = torch.as_tensor(ids).long()
    S = ids.shape[1]
    causal = torch.full((S, S), float("-inf"), dtype=dtype).triu(1)
    cross_mask = encoder_key_mask(frames, enc.shape[1], dtype)
    h = prenet(ids, sd, dtype)
    p_self, p_cross = [], []
    for l in range(num_layers(sd)):
        lp = f"{DEC}{l}."
        sk, sv = project_kv(h, sd, lp + "self_attn.", dtype)
        ck, cv = project_kv(enc, sd, lp + "encoder_attn.", dtype)
        a, ps = _attend(h, sk, sv, causal, sd, lp + "self_attn.", dtype)
        h = _ln(h + a, sd, lp + "self_attn_layer_norm", dtype)
        a, pc = _attend(h, ck, cv, cross_mask, sd, lp + "encoder_attn.", dtype)
        h = _ln(h + a, sd, lp + "encoder_attn_layer_norm", dtype)
        f = gelu_erf(F.linear(h, _t(sd, lp + "feed_forward.intermediate_dense.weight", dtype), _t(sd, lp + "feed_forward.intermediate_dense.bias", dtype)))
        f = F.linear(f, _t(sd, lp + "feed_forward.output_dense.weight", dtype), _t(sd, lp + "feed_forward.output_dense.bias", dtype))
        h = _ln(h + f, sd, lp + "final_layer_norm", dtype)
        p_self.append(ps)
        p_cross.append(pc)
    return F.linear(h, _t(sd, "text_decoder_postnet.lm_head.weight", dtype)), p_self, p_cross


def mean_attention(p_cross, pairs=None):
    """A [B,S,T]: the mean of P_cross[l][:, h] over ``pairs`` ((layer, head); None = all)."""
    if pairs is None:
        pairs = [(l, h) for l in range(len(p_cross)) for h in range(p_cross[l].shape[1])]
    acc = torch.zeros_like(p_cross[0][:, 0])
    for l, h in sorted(pairs):
        acc = acc + p_cross[l][:, h]
    return acc / len(pairs)


def dtw(A):
    """Monotone DTW over the cost -A (float64 [n, F]) from (0, 0) to (n-1, F-1): D[s,t] = c[s,t] + min(D[s-1,t-1], D[s-1,t],
    D[s,t-1]), ties diagonal first, then (s-1,t), then (s,t-1).  Returns (start [n], end [n], path [(s, t)] from the origin)."""
    c = -np.asarray(A, dtype=np.float64)
    n, Fr = c.shape
    D = np.full((n, Fr), np.inf)
    bp = np.zeros((n, Fr), dtype=np.uint8)
    inf = np.inf
    for s in range(n):
        for t in range(Fr):
            if s == 0 and t == 0:
                D[0, 0] = c[0, 0]
                continue
            best, frm = (D[s - 1, t - 1] if s > 0 and t > 0 else inf), 0
            up = D[s - 1, t] if s > 0 else inf
            left = D[s, t - 1] if t > 0 else inf
            if up < best:
                best, frm = up, 1
            if left < best:
                best, frm = left, 2
            D[s, t] = c[s, t] + best
            bp[s, t] = frm
    s, t = n - 1, Fr - 1
    path = [(s, t)]
    while s > 0 or t > 0:
        frm = bp[s, t]
        if frm == 0:
            s, t = s - 1, t - 1
        elif frm == 1:
            s -= 1
        else:
            t -= 1
        path.append((s, t))
    path.reverse()
    start, end = np.full(n, Fr, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for s, t in path:
        start[s] = min(start[s], t)
        end[s] = max(end[s], t + 1)
    return start, end, path


def dtw_batch(A, counts, frames):
    """``dtw`` per clip on A [B,S,T] (the float32 values as given, widened): (start, end) i32 [B,S], -1 for s >= counts[b]."""
    A = np.asarray(A)
    B, S, T = A.shape
    start, end = np.full((B, S), -1, dtype=np.int32), np.full((B, S), -1, dtype=np.int32)
    for b in range(B):
        n, Fr = int(counts[b]), int(T if frames is None else frames[b])
        if n > 0 and Fr > 0:
            start[b, :n], end[b, :n], _ = dtw(A[b, :n, :Fr])
    return start, end
