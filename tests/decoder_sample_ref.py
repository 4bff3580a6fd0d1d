"""CPU restatement of the decoder's sampling rule (include/loco_asr.h, csrc/decoder_sample.hip), for tests only; no GPU, no library.

``philox4x32_10`` / ``uniform`` are the generator in Python integers (exact).  ``keep_mask`` and ``draw`` restate steps 1-3 and 5 of the
rule in float64 (or in the dtype given) and hand out the quantities a test needs to leave out what no fp32 implementation can be held
to: every column's cumulative mass A_i beside the threshold 1 - top_p, and the draw's normalised prefix boundaries beside u."""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """The four output words of Philox4x32-10 (Salmon et al., SC'11) for a 4-word counter and a 2-word key."""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, utterance, hypothesis, t):
    """u of the rule's step 4 as a Python float (exact: 24 bits)."""
    x0 = philox4x32_10((utterance, hypothesis, t, 0), (seed & MASK, (seed >> 32) & MASK))[0]
    return (x0 >> 8) * 2.0 ** -24


def argmax_rule(row):
    """decoder_common.h's argmax: the first NaN wins, otherwise the largest value, the lowest index on a tie."""
    row = torch.as_tensor(row)
    nan = torch.isnan(row)
    if bool(nan.any()):
        return int(nan.nonzero()[0])
    return int((row == row.max()).nonzero()[0])


def degenerate(row, temperature=1.0):
    """Step 6: a NaN, a +inf maximum or nothing but -inf, of z = row / temperature in fp32."""
    row = torch.as_tensor(row, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)
    return bool(torch.isnan(row).any()) or not bool(torch.isfinite(row.max()))


def keep_mask(row, temperature, top_k, top_p, dtype=torch.float64):
    """Steps 1-3 on one row of fp32 logits: (keep bool [V], A [V] -- the cumulative mass of every top-k survivor, NaN elsewhere).  The
    division is the rule's fp32 one; everything after it runs in ``dtype``."""
    row = torch.as_tensor(row, dtype=torch.float32)
    V = row.shape[0]
    z = (row / torch.tensor(temperature, dtype=torch.float32)).to(dtype)
    k = V if top_k == 0 else min(int(top_k), V)
    above = (z[None, :] > z[:, None]).sum(1)
    surv = above < k
    A = torch.full((V,), float("nan"), dtype=dtype)
    keep = surv.clone()
    if top_p < 1:
        w = torch.where(surv, torch.exp(z - z.max()), torch.zeros((), dtype=dtype))
        p = w / w.sum()
        A = torch.where(surv, ((z[None, :] <= z[:, None]) * p[None, :]).sum(1), A)
        keep = surv & (A > 1 - torch.tensor(top_p, dtype=torch.float32).to(dtype))
        keep[argmax_rule(row)] = True
    return keep, A


def draw(row, temperature, keep, u, dtype=torch.float64):
    """Step 5: (token, the distance of u from the nearest normalised prefix boundary of a kept column, probabilities [V])."""
    row = torch.as_tensor(row, dtype=torch.float32)
    z = (row / torch.tensor(temperature, dtype=torch.float32)).to(dtype)
    w = torch.where(keep, torch.exp(z - z.max()), torch.zeros((), dtype=dtype))
    pre = torch.cumsum(w, 0)
    Z = pre[-1]
    over = (keep & (pre > u * Z)).nonzero()
    token = int(over[0]) if over.numel() else int(keep.nonzero()[-1])
    edges = (pre / Z)[keep]
    return token, float((edges - u).abs().min()), w / Z


def sample_row(row, temperature, top_k, top_p, seed, utterance, hypothesis, t, greedy=False):
    """The whole rule in float64: the token of one row."""
    if greedy or degenerate(row, temperature):
        return argmax_rule(row)
    keep, _ = keep_mask(row, temperature, top_k, top_p)
    return draw(row, temperature, keep, uniform(seed, utterance, hypothesis, t))[0]


def counters(utterance, hypothesis, t):
    """u32 [M, 3] for rows that share nothing: broadcast of the three."""
    u, h, t = np.broadcast_arrays(np.asarray(utterance, np.uint32), np.asarray(hypothesis, np.uint32), np.asarray(t, np.uint32))
    return np.stack([u, h, t], -1).astype(np.uint32)


# ---- the same on [M, V] blocks (sorting instead of the O(V^2) comparisons; tests/test_decoder_sample_host.py pins it to the per-row form)
def scaled(rows, temperature):
    """z = rows / temperature, the rule's fp32 division, as float64."""
    return (torch.as_tensor(rows, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)).double()


def keep_mask_rows(rows, temperature, top_k, top_p):
    """``keep_mask`` for every row of a block without NaN: (keep bool [M, V], A f64 [M, V], NaN where top-k removed the column or
    top_p is 1)."""
    z = scaled(rows, temperature)
    M, V = z.shape
    k = V if top_k == 0 else min(int(top_k), V)
    order = torch.sort(z, dim=1).values
    upto = torch.searchsorted(order, z.contiguous(), right=True)  # columns with z_j <= z_i
    surv = (V - upto) < k
    A = torch.full((M, V), float("nan"), dtype=torch.float64)
    keep = surv.clone()
    if top_p < 1:
        w = torch.where(surv, torch.exp(z - z.max(1, keepdim=True).values), torch.zeros((), dtype=torch.float64))
        p = w / w.sum(1, keepdim=True)
        p_sorted = torch.gather(p, 1, torch.argsort(z, dim=1, stable=True))
        cum = torch.cumsum(p_sorted, 1)
        A = torch.where(surv, torch.gather(cum, 1, upto - 1), A)
        keep = surv & (A > 1 - float(np.float32(top_p)))
        keep[torch.arange(M), torch.as_tensor([argmax_rule(r) for r in torch.as_tensor(rows)])] = True
    return keep, A


def draw_rows(rows, temperature, keep, u):
    """``draw`` for every row: (tokens i64 [M], margin f64 [M] = the distance of u from the nearest prefix boundary of a kept column,
    probabilities f64 [M, V])."""
    z = scaled(rows, temperature)
    u = torch.as_tensor(u, dtype=torch.float64)[:, None]
    w = torch.where(keep, torch.exp(z - z.max(1, keepdim=True).values), torch.zeros((), dtype=torch.float64))
    pre = torch.cumsum(w, 1)
    Z = pre[:, -1:]
    over = keep & (pre > u * Z)
    V = z.shape[1]
    first = torch.where(over, torch.arange(V)[None, :], V).min(1).values
    last = torch.where(keep, torch.arange(V)[None, :], -1).max(1).values
    margin = torch.where(keep, (pre / Z - u).abs(), torch.full((), float("inf"), dtype=torch.float64)).min(1).values
    return torch.where(first < V, first, last), margin, w / Z


def reference_error(rows, temperature):
    """e_torch: the largest difference between torch's CPU fp32 softmax, and its cumsum, and float64 on the same rows."""
    z32 = torch.as_tensor(rows, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)
    p32, p64 = torch.softmax(z32, 1), torch.softmax(z32.double(), 1)
    return max(float((p32.double() - p64).abs().max()), float((torch.cumsum(p32, 1).double() - torch.cumsum(p64, 1)).abs().max()))


def chi2_quantile(q, dof):
    """The q quantile of the chi-square distribution with ``dof`` degrees of freedom (bisection on the regularised incomplete gamma)."""
    cdf = lambda x: float(torch.special.gammainc(torch.tensor(dof / 2.0, dtype=torch.float64), torch.tensor(x / 2.0, dtype=torch.float64)))  # noqa: E731
    lo, hi = 0.0, 10.0 * dof + 200.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < q else (lo, mid)
    return hi
