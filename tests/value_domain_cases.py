"""Hostile inputs, and their plain references, shared by tests/test_value_domain_ref.py (CPU), tests/test_gpu_value_domain.py and
tests/test_gpu_softmax_hostile.py.  Pure numpy / torch-CPU: nothing here imports the library.

* GELU: a grid that reaches the clamp at |x| = 5.79827547, the subnormals and the specials; the float64 reference in its erfc form
  (no cancellation in the negative tail); the polynomial of csrc/loco_kernels.h restated in float32 with an exact exp2.
* the fp16 plane split: every fp16 number, every tie between two neighbours, the ties' fp32 neighbours, the 65504 / 65520 edge;
  expected_split is the definition the header gives, evaluated by torch's round-to-nearest-even conversions.
* online softmaxes: inputs on which the running maximum rises late, in every tile, or never; LayerNorm rows far from N(0, 1).
"""
import math

import numpy as np
import torch

F32 = np.float32
K_SMAX = F32(5.79827547)  # the clamp of gelu_erf: 4.1 sqrt(2)

# ---- bars of the GELU tests (tests/test_gpu_value_domain.py asserts them, tests/test_value_domain_ref.py checks their constants) ---------
# Each is the restatement's CPU figure, rounded up (RESTATED_*, asserted by the CPU test) plus what the 1 ulp of v_exp_f32 on h = erfc / 2
# can add: h <= 1/2, so (1 - h) moves by at most 2^-24 / (1/2) = 2^-23 relative (x > 0), and x h by 2^-24 |x| absolute (x < 0).
RESTATED_POS_REL = 1.7e-7      # x > 0, relative                (quoted 1.64e-7; this restatement: 1.27e-7)
RESTATED_NEG_REL = 3.3e-6      # -5.7 <= x < 0, relative        (quoted 3.2e-6; this restatement: 2.6e-6)
RESTATED_TAIL_ABS = 2.0e-8     # x < -5.7, absolute             (quoted 1.95e-8; this restatement: 1.94e-8)
RESTATED_NEG_ABS_PER_X = 6.0e-8  # x < 0, absolute error / |x|  (quoted 5.8e-8)
BAR_POS_REL = 3e-7
BAR_NEG_REL = 4e-6
BAR_TAIL_ABS = 2.5e-8
TAIL = -5.7
# A result below FLT_MIN is a multiple of 2^-149: no relative bar can be met there, whatever the kernel does.  One such quantum is
# added to every relative bar (it is 4e-8 of the smallest normal number and nothing above it).
SUBNORMAL_QUANTUM = 2.0 ** -149


def _neighbours(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def gelu_grid():
    """(finite fp32 grid, specials): linspace(-9, 9), +-2^k, +-0 and its neighbours, the clamp and its neighbours, the range's ends."""
    g = [np.linspace(-9.0, 9.0, 4096, dtype=np.float64).astype(F32)]
    pw = np.asarray([2.0 ** k for k in range(-40, 5)], F32)
    g += [pw, -pw, np.asarray([0.0, -0.0], F32)]
    g += [np.asarray(_neighbours(0.0), F32)]
    edge = np.asarray(_neighbours(K_SMAX), F32)
    g += [edge, -edge]
    tiny = np.asarray([np.finfo(F32).tiny, 2.0 ** -149, 1e30], F32)
    g += [tiny, -tiny]
    specials = np.asarray([np.inf, -np.inf, np.nan], F32)
    return np.concatenate(g).astype(F32), specials


def gelu_subgrid(n):
    """n grid points for a path that sees few values: the edges first, then an even sample of the linspace."""
    grid, _ = gelu_grid()
    edges = grid[4096 + 90:]               # +-0, the neighbours of 0, the clamp's neighbourhood, FLT_MIN, the subnormal, 1e30
    pw = grid[4096:4096 + 90][::6]         # every sixth power of two, both signs
    rest = n - len(edges) - len(pw)
    assert rest >= 200
    lin = grid[np.linspace(0, 4095, rest).round().astype(int)]
    return np.concatenate([edges, pw, lin]).astype(F32)


def gelu_ref64(x):
    """0.5 x erfc(-x / sqrt 2) in float64; the limits at the infinities (0 and +inf), NaN for NaN."""
    x = torch.as_tensor(np.asarray(x, np.float64))
    fin = torch.isfinite(x)
    y = 0.5 * torch.where(fin, x, torch.zeros_like(x)) * torch.erfc(-torch.where(fin, x, torch.zeros_like(x)) / math.sqrt(2.0))
    y = torch.where(x == float("inf"), x, y)
    y = torch.where(x == float("-inf"), torch.zeros_like(x), y)
    y = torch.where(torch.isnan(x), x, y)
    return y.numpy()


_Q = [2.171883651e-08, -6.759613029e-07, 9.013814633e-06, -6.522983313e-05, 2.421164681e-04, 7.379760791e-05, -7.028903347e-03,
      5.248807371e-02, 4.592096508e-01, 1.151104808e+00]


def _fma32(a, b, c):
    """fmaf: the product of two fp32 numbers is exact in float64, the sum is rounded to float64 and then to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def gelu_restated32(x, last_coefficient=None):
    """gelu_erf of csrc/loco_kernels.h, operation by operation in fp32, with exp2 correctly rounded instead of v_exp_f32."""
    x = np.asarray(x, F32)
    coef = [F32(c) for c in _Q]
    if last_coefficient is not None:
        coef[-1] = F32(last_coefficient)
    with np.errstate(all="ignore"):
        s = np.fmin(np.abs(x), K_SMAX)  # fminf: a NaN operand gives the other one
        q = np.full_like(s, coef[0])
        for c in coef[1:]:
            q = _fma32(q, s, np.full_like(s, c))
        u = (q * s).astype(F32)
        h = (F32(0.5) * np.exp2(-u.astype(np.float64)).astype(F32)).astype(F32)
        pos = (x * (F32(1.0) - h).astype(F32)).astype(F32)
        neg = (np.where(x < -K_SMAX, -K_SMAX, x).astype(F32) * h).astype(F32)
        return np.where(x >= 0, pos, neg).astype(F32)


def gelu_errors(x, got):
    """Worst figures of `got` against gelu_ref64 over the finite x, in the four regions the bars name (region -> (figure, at x))."""
    x = np.asarray(x, F32)
    ref = gelu_ref64(x)
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        above = np.maximum(err - SUBNORMAL_QUANTUM, 0.0)
        rel = above / np.abs(ref)
        per_x = above / np.abs(x.astype(np.float64))
    out = {}
    for name, sel, fig in (("pos_rel", x > 0, rel), ("neg_rel", (x < 0) & (x >= TAIL), rel), ("tail_abs", x < TAIL, err),
                           ("neg_abs_per_x", x < 0, per_x)):
        sel = sel & np.isfinite(x)
        if not sel.any():
            continue
        f = np.where(sel, fig, -1.0)
        i = int(np.nanargmax(f))
        assert not np.isnan(f[sel]).any(), name
        out[name] = (float(f[i]), float(x[i]))
    return out


# ---- the fp16 plane split ---------------------------------------------------------------------------------------------------------------
SPLIT_ROWS, SPLIT_COLS = 256, 1024


def expected_split(x):
    """(hi, lo) = (fp16(x), fp16(x - (float)hi)), round to nearest even: the definition in csrc/loco_kernels.h."""
    x = torch.as_tensor(x, dtype=torch.float32)
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


def split_specials():
    f = [65504.0, float(np.nextafter(F32(65520.0), F32(0.0))), 65520.0, 1e5, float("inf"), float("nan")]
    f += [2.0 ** -149, 2.0 ** -140, float(np.nextafter(np.finfo(F32).tiny, F32(0.0))), float(np.finfo(F32).tiny)]
    f += [2.0 ** -k for k in range(15, 41)]
    f = np.asarray(f, F32)
    return np.concatenate([f, -f, np.asarray([0.0, -0.0], F32)])


def split_ties():
    """The midpoints of neighbouring fp16 numbers from (0, h_1) to (h_last-1, 65504), positive: exact in fp32."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)  # 0, every finite positive fp16 number
    mid = ((h[:-1] + h[1:]) / 2).astype(F32)
    assert np.array_equal(mid.astype(np.float64), (h[:-1] + h[1:]) / 2)
    return mid


def split_values():
    """fp32 [256, 1024]: the specials, then every finite fp16 number, every tie and each tie's two fp32 neighbours, both signs; padded
    with 1.0."""
    h = np.arange(1, 0x7C00, dtype=np.uint16).view(np.float16).astype(F32)
    mid = split_ties()
    pos = np.concatenate([h, mid, np.nextafter(mid, F32(-np.inf)), np.nextafter(mid, F32(np.inf))]).astype(F32)
    v = np.concatenate([split_specials(), pos, -pos]).astype(F32)
    assert v.size <= SPLIT_ROWS * SPLIT_COLS
    out = np.ones(SPLIT_ROWS * SPLIT_COLS, F32)
    out[:v.size] = v
    return out.reshape(SPLIT_ROWS, SPLIT_COLS)


def split_narrow_values(rows, cols):
    """fp32 [rows, cols] for a path that sees few values: the specials, then ties (with both fp32 neighbours) sampled evenly."""
    mid = split_ties()
    n = rows * cols
    sp = split_specials()
    k = (n - sp.size) // 6
    m = mid[np.linspace(0, mid.size - 1, k).round().astype(int)]
    pos = np.concatenate([m, np.nextafter(m, F32(-np.inf)), np.nextafter(m, F32(np.inf))])
    v = np.concatenate([sp, pos, -pos]).astype(F32)
    out = np.ones(n, F32)
    out[:v.size] = v
    return out.reshape(rows, cols)


def ulp_f16(h):
    """Spacing of fp16 at |h| (2^-24 in the subnormals), float64."""
    a = np.abs(np.asarray(h, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def hi_is_nearest(hi, lo):
    """True where hi is a nearest fp16 number to hi + lo.  (half(hi + lo) == hi is that, except where hi + lo is exactly a tie: x one
    fp32 step beside a tie has lo rounded to half a spacing exactly, and the tie may then round to hi's neighbour.)  torch fp16."""
    hi, lo = torch.as_tensor(hi), torch.as_tensor(lo)
    rec = hi.double() + lo.double()
    bits = hi.view(torch.int16).int()
    mag = bits & 0x7FFF
    up = torch.where(mag < 0x7BFF, mag + 1, mag)      # neighbours in magnitude (the one above 65504 does not exist: hi itself)
    dn = torch.where(mag > 0, mag - 1, mag + 1)       # ... below 0: the smallest number of the other sign, by symmetry the same distance
    sign = torch.where(bits < 0, -1.0, 1.0).double()
    f = lambda m: m.to(torch.int16).view(torch.float16).double() * sign  # noqa: E731
    d = (rec - hi.double()).abs()
    return (d <= (rec - f(up)).abs()) & (d <= (rec - torch.where(mag > 0, f(dn), -f(dn))).abs())


def split_bound(x):
    """|x - (hi + lo)| of a correct split, from the format: 22 bits, levelling off at 2^-25 where lo is subnormal."""
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(x, np.float64)), 2.0 ** -25)


# ---- the bar of the softmax and LayerNorm tests -------------------------------------------------------------------------------------------
def row_bar(ref64, torch32):
    """Per element: max(4 x the row's largest error of torch's CPU fp32 evaluation against float64, 2^-21 max(1, |ref|)) -- the rule of
    tests/test_gpu_decoder_score.py.  Rows are the last axis."""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    e = (torch.as_tensor(torch32).double() - ref64).abs().amax(-1, keepdim=True)
    return torch.maximum(4 * e, 2.0 ** -21 * ref64.abs().clamp(min=1.0))


def worst_ratio(got, ref64, bar):
    got = torch.as_tensor(got).double().cpu()
    return float(((got - ref64).abs() / bar).max())


# ---- decoder attention ------------------------------------------------------------------------------------------------------------------
HEADS, HEAD_DIM, SCALE = 12, 64, 0.125
LEAD = 30.0
ASCENT = 2.0
ATTN_KINDS = ["lead599", "lead256", "lead63", "lead64", "ascending", "equal"]  # the lead's key is clipped to Tk - 1 where Tk is shorter


def _unit_directions(g):
    u = torch.randn((HEADS, HEAD_DIM), generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def _planted(g, rows_q, Tk, B=1):
    """q, k float64 [B, rows, 12, 64] with scores SCALE q.k of order one, q with component 8 along a per-head unit direction u and k with
    none: adding c u to key j then raises that key's score by exactly c for every query of the head."""
    u = _unit_directions(g)
    q = torch.randn((B, rows_q, HEADS, HEAD_DIM), generator=g, dtype=torch.float64)
    k = torch.randn((B, Tk, HEADS, HEAD_DIM), generator=g, dtype=torch.float64)
    q = q - (q * u).sum(-1, keepdim=True) * u + 8.0 * u
    k = k - (k * u).sum(-1, keepdim=True) * u
    return q, k, u


def _plant_kind(kind, q, k, u):
    Tk = k.shape[1]
    base = float((SCALE * torch.einsum("bihd,bjhd->bhij", q, k)).abs().max())
    if kind.startswith("lead"):
        j = min(int(kind[4:]), Tk - 1)
        k[:, j] += (LEAD + 2 * base) * u                  # its own base score is >= -base, the others' <= base: it leads by LEAD ... LEAD + 4 base
    elif kind == "last":
        k[:, Tk - 1] += (LEAD + 2 * base) * u
    elif kind == "ascending":                             # ASCENT / 64 nats per key, the base scaled down to a fifth of that: strictly ascending
        step = ASCENT / 64.0
        k = (0.2 * step / base) * k + step * torch.arange(Tk, dtype=torch.float64)[None, :, None, None] * u
    elif kind == "equal":
        k = k[:, :1].expand(-1, Tk, -1, -1).clone()
    else:
        raise ValueError(kind)
    return k


def decoder_attention_case(kind, Sq, Tk, seed=0):
    """q [1, Sq, 768], k, v [1, Tk, 768] fp32.  lead<j>: key j outscores every key by about LEAD nats for every query and head;
    ascending: the score rises by ASCENT nats per tile of 64 keys and the base is scaled down to a fifth of the step between two keys,
    so the scores ascend strictly in j and every tile, a last one of a single key included, raises the running maximum;
    equal: every key is the same vector (a uniform softmax: the output is the mean of v)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Tk + Sq)
    q, k, u = _planted(g, Sq, Tk)
    k = _plant_kind(kind, q, k, u)
    v = torch.randn((1, Tk, HEADS * HEAD_DIM), generator=g, dtype=torch.float64)
    return q.reshape(1, Sq, 768).float(), k.reshape(1, Tk, 768).float(), v.float()


def attention_ref(q, k, v, counts, causal, offset, dtype=torch.float64):
    """softmax_j(SCALE q.k) v over keys j < counts[b] and, when causal, j <= i + offset; [B, Sq, 768] in `dtype` on the CPU."""
    B, Sq, _ = q.shape
    Tk = k.shape[1]
    qh, kh, vh = (t.to(dtype).view(B, -1, HEADS, HEAD_DIM).transpose(1, 2) for t in (q, k, v))
    s = (qh * SCALE) @ kh.transpose(-1, -2)
    return (torch.softmax(s.masked_fill(~visible(B, Sq, Tk, counts, causal, offset)[:, None], float("-inf")), -1) @ vh).transpose(1, 2).reshape(B, Sq, 768)


def visible(B, Sq, Tk, counts, causal, offset):
    j = torch.arange(Tk)
    counts = torch.full((B,), Tk) if counts is None else torch.as_tensor(counts)
    vis = (j[None, None, :] < counts[:, None, None]).expand(B, Sq, Tk)
    if causal:
        vis = vis & (j[None, None, :] <= torch.arange(Sq)[None, :, None] + offset)
    return vis


PROBS_KINDS = ["last", "ascending"]


def decoder_probs_case(kind, B, Sq, Tk, seed=0):
    """q [B, Sq, 768], k [B, Tk, 768] fp32 for the probabilities kernel: the leading key is the last one (the row's last tile)."""
    g = torch.Generator().manual_seed(2000 * seed + 7 * Tk + Sq + 31 * B)
    q, k, u = _planted(g, Sq, Tk, B)
    k = _plant_kind(kind, q, k, u)
    return q.reshape(B, Sq, 768).float(), k.reshape(B, Tk, 768).float()


def probs_ref(q, k, counts, causal, dtype=torch.float64):
    """(P [B, 12, Sq, Tk] in `dtype`, visible [B, 12, Sq, Tk])."""
    B, Sq, _ = q.shape
    Tk = k.shape[1]
    qh, kh = (t.to(dtype).view(B, -1, HEADS, HEAD_DIM).transpose(1, 2) for t in (q, k))
    vis = visible(B, Sq, Tk, counts, causal, 0)[:, None].expand(B, HEADS, Sq, Tk)
    return torch.softmax(((qh * SCALE) @ kh.transpose(-1, -2)).masked_fill(~vis, float("-inf")), -1), vis


# ---- intent head: attention pooling -----------------------------------------------------------------------------------------------------
def head_query(seed=0):
    """The learned query at the scale the head's own tests use (300 x its initial 1e-3): fp32 [768]."""
    g = torch.Generator().manual_seed(50 + seed)
    return (torch.randn(768, generator=g) * 0.3).float()


def head_batch(T, q, seed=0):
    """x fp32 [3, T, 768] and one-hot targets [3, 101].  The component of every frame along q is replaced, so z_t = x_t . q is, to fp32
    rounding: clip 0 ascending from 0 to 24 (every 128-frame split raises the maximum), clip 1 order one with the last frame (the last
    split; at T = 129 a split of that one frame) leading by 30, clip 2 order one with frame T // 3 leading by 80 (every other weight
    is below 2^-115 and vanishes from every fp32 sum)."""
    g = torch.Generator().manual_seed(3000 * seed + T)
    qd = q.double()
    x = torch.randn((3, T, 768), generator=g, dtype=torch.float64) * 0.8
    x = x - (x @ qd)[..., None] * qd / (qd @ qd)
    z = torch.randn((3, T), generator=g, dtype=torch.float64)
    z[0] = torch.linspace(0.0, 24.0, T, dtype=torch.float64)
    z[1, T - 1] = z[1].max() + 30.0
    z[2, T // 3] = z[2].max() + 80.0
    x = x + z[..., None] * qd / (qd @ qd)
    cls = torch.tensor([3, 57, 100])
    return x.float(), torch.eye(101, dtype=torch.int64)[cls]


def head_reference(oracle_cls, q, W, b, x, target, dtype):
    """logits [3, 101], loss, dW, db, dq of the attention-pooling head in `dtype` by torch autograd on the CPU."""
    m = oracle_cls("attention").to(dtype)
    with torch.no_grad():
        m.q.copy_(q.to(dtype)[None])
        m.classifier[0].weight.copy_(W.to(dtype))
        m.classifier[0].bias.copy_(b.to(dtype))
    pred = m(x.to(dtype))
    loss = torch.nn.CrossEntropyLoss()(pred.squeeze(1), target.to(dtype))
    loss.backward()
    return dict(logits=pred.detach().squeeze(1), loss=loss.detach().reshape(1), dW=m.classifier[0].weight.grad, db=m.classifier[0].bias.grad[None],
                dq=m.q.grad.reshape(1, -1))


def head_params(seed=0):
    g = torch.Generator().manual_seed(70 + seed)
    return (torch.randn((101, 768), generator=g) * 0.05).float(), (torch.randn(101, generator=g) * 0.1).float()


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------
def layernorm_rows(dim, seed=0):
    """x fp32 [5, dim], gamma, beta: mean 1e3 with unit spread; one channel at 1e4 among N(0, 1) (a massive activation); spread 1e-4
    around 0 (eps = 1e-5 dominates the variance 1e-8); two benign rows."""
    g = torch.Generator().manual_seed(90 + dim + seed)
    x = torch.randn((5, dim), generator=g)
    x[0] += 1e3
    x[1, dim // 3] = 1e4
    x[2] *= 1e-4
    x[3] = x[3] * 3.0 + 0.5
    x[4] = x[4] * 0.1 - 2.0
    gamma = torch.rand(dim, generator=g) + 0.5
    beta = torch.rand(dim, generator=g) - 0.5
    return x.float(), gamma.float(), beta.float()


def layernorm_ref(x, gamma, beta, dtype):
    return torch.nn.functional.layer_norm(x.to(dtype), (x.shape[-1],), gamma.to(dtype), beta.to(dtype), 1e-5)
