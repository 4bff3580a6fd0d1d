"""Cases, operands and fp64 references of the decoder's per-element contract, shared by tests/test_gpu_decoder_contract.py (the kernels)
and tests/test_decoder_contract_ref.py (fp32 restatements and their mutations, on the CPU).  Pure torch-CPU: nothing here imports the
library.  Every reference is built once per case (functools.lru_cache) and never modified.

Skinny GEMM.  ks = op_check.skinny_slices(N, K) k-slices, cols = (4 / ks) * 2 columns per workgroup; for each slicing N = cols - 1, cols,
cols + 1 and a larger N that is no multiple of cols, N = 1, every K at which the slicing or its evenness changes (256: one slice; 512, 768:
two; 1024: four at N = 128, two at N = 132; 1280 at N = 81: four uneven slices of 2, 1, 1, 1 chunks; 2048, 3072: four), M around the 4-row
register pass and the 64-row limit, the three epilogues, a null bias.

Attention.  Shapes by what dec_attention_splits makes of them (op_check.dec_attention_splits restates it), values in three families:
  flat       q, k ~ N(0, 1): scores of order one, every key carries weight;
  ascending  value_domain_cases' planted ascent, 2 nats per tile of 64 keys: every tile and every split raises the running maximum, the
             last keys of a row carry the weight;
  late       the key that begins the last tile of the row's visible range leads by 6 to 10 nats over scores within +-1: the maximum arrives
             in the last tile of the last non-empty split and everything summed before it is rescaled by e^-6 or less, yet the other
             keys together still carry a few percent of the output (a lead of 30 nats would leave out = v of that key, bit for bit, and an
             error of 0 whatever the kernel did with the rest).  Where the visible range differs from query to query (causal), the key
             is placed for the LAST query; earlier queries then see a flat row.
"""
import functools

import torch

import value_domain_cases as vd

HEADS, HD, HID = 12, 64, 768
FAMILIES = ("flat", "ascending", "late")
LATE_LEAD = 6.0

# ---- skinny GEMM ------------------------------------------------------------------------------------------------------------------------
# (M, N, K, epilogue, bias)
GEMM_CASES = [
    (1, 7, 256, 0, True), (3, 8, 256, 1, True), (4, 9, 256, 2, False), (5, 77, 256, 0, True), (1, 1, 256, 1, True),      # one slice, cols 8
    (63, 3, 512, 1, True), (64, 4, 512, 2, True), (1, 5, 768, 0, False), (5, 81, 768, 2, True), (64, 1, 768, 0, True),   # two slices, cols 4
    (64, 2304, 768, 0, True), (3, 132, 1024, 1, True),
    (4, 128, 1024, 0, True), (63, 81, 1280, 2, True), (5, 81, 1280, 1, False),                                          # four slices, cols 2
    (1, 1, 2048, 0, True), (3, 2, 2048, 2, True), (64, 3, 2048, 1, True), (4, 771, 3072, 0, True), (63, 768, 3072, 2, False),
]


def gemm_id(case):
    M, N, K, epi, bias = case
    return f"M{M}-N{N}-K{K}-e{epi}" + ("" if bias else "-nobias")


def _uniform(g, shape, scale):
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


@functools.lru_cache(maxsize=None)
def gemm_operands(M, N, K):
    """A [M, K], W [N, K], bias [N], R [M, N] fp32 on the CPU: |A W^T| of order one"""
    g = torch.Generator().manual_seed(100003 * M + 101 * N + K)
    return _uniform(g, (M, K), 1.7), _uniform(g, (N, K), 2.0 / K ** 0.5), _uniform(g, (N,), 0.3), _uniform(g, (M, N), 1.0)


# ---- attention --------------------------------------------------------------------------------------------------------------------------
# name -> B, Sq, Tk, counts (None: Tk), causal, offset.  Splits as dec_attention_splits gives them.
ATTN_CASES = {
    # two splits of 192 and 65 keys: counts at the first split's end, one below, one above, and the whole range
    "split2-191": (1, 1, 257, [191], 0, 0), "split2-192": (1, 1, 257, [192], 0, 0), "split2-193": (1, 1, 257, [193], 0, 0),
    "split2-257": (1, 1, 257, [257], 0, 0),
    # three splits of 256: empty trailing splits, a middle split, every count around a split's end
    "split3": (7, 1, 600, [1, 255, 256, 257, 512, 513, 600], 0, 0),
    # 4320 rows: one split, five tiles
    "single": (3, 120, 300, [300, 129, 64], 0, 0),
    # three splits, the visible count goes 254, 255, 256, 257, 258 from query to query: across the first split's end
    "causal-cross": (1, 5, 600, None, 1, 253),
    # the language model's: causal self-attention, counts = the rows' lengths; S = 300 has two splits of 192, S = 130 one
    "lm-300": (1, 300, 300, [300], 1, 0), "lm-130": (2, 130, 130, [130, 77], 1, 0),
    # counts of 0, below 0 and above Tk, split and unsplit
    "counts-split": (4, 1, 257, [0, -5, 1000, 257], 0, 0), "counts-single": (4, 2, 100, [0, -1, 101, 3], 0, 0),
    # a negative offset: queries 0 .. 2 see no key at all, query 3 sees key 0; two splits, and one
    "no-keys-split": (1, 6, 300, None, 1, -3), "no-keys-single": (2, 6, 70, [70, 2], 1, -3),
}
FUSED_CASES = ("lm-300", "lm-130")  # Sq == Tk: q, k and v can be the columns of one [B, S, 2304] buffer


def visible_counts(B, Sq, Tk, counts, causal, offset):
    """int64 [B, Sq]: visible keys of every query, the rule of decoder_common.h (dec_visible_keys), never below 0"""
    n = torch.full((B,), Tk) if counts is None else torch.as_tensor(counts).clamp(max=Tk)
    n = n[:, None].expand(B, Sq)
    if causal:
        n = torch.minimum(n, torch.arange(Sq)[None] + offset + 1)
    return n.clamp(min=0)


def heads(x):
    """[B, T, 768] -> [B, 12, T, 64]"""
    return x.view(x.shape[0], x.shape[1], HEADS, HD).transpose(1, 2)


def unheads(x):
    """[B, 12, T, 64] -> [B, T, 768]"""
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], HID)


def attn_values(family, B, Sq, Tk, nvis, seed=0):
    """q [B, Sq, 768] (to be used with scale vd.SCALE), k, v [B, Tk, 768] fp32; nvis [B, Sq] from visible_counts"""
    g = torch.Generator().manual_seed(7919 * seed + 31 * B + 7 * Tk + Sq + 1000 * FAMILIES.index(family))
    if family == "flat":
        q = torch.randn((B, Sq, HEADS, HD), generator=g, dtype=torch.float64) / vd.SCALE ** 0.5 / HD ** 0.25
        k = torch.randn((B, Tk, HEADS, HD), generator=g, dtype=torch.float64) / vd.SCALE ** 0.5 / HD ** 0.25
    else:
        q, k, u = vd._planted(g, Sq, Tk, B)
        if family == "ascending":
            k = vd._plant_kind("ascending", q, k, u)
        else:
            k = k / float((vd.SCALE * torch.einsum("bihd,bjhd->bhij", q, k)).abs().max())  # every score now within +-1
            for b in range(B):
                n = int(nvis[b, -1])
                if n > 0:
                    k[b, 64 * ((n - 1) // 64)] += (LATE_LEAD + 2.0) * u               # ... and this one ahead by LATE_LEAD to LATE_LEAD + 4
    v = torch.randn((B, Tk, HID), generator=g, dtype=torch.float64)
    return q.reshape(B, Sq, HID).float(), k.reshape(B, Tk, HID).float(), v.float()


def attn_reference(q, k, v, nvis, scale):
    """fp64 reference of softmax_j(scale q . k) v over the keys j < nvis[b, i], and what the bar needs.  Everything [B, 12, Sq, 64] or
    [B, 12, Sq, 1]: ref, S = sum_j w |v|, A_max, spread_max, nvis (float64), has_keys (bool)."""
    qh, kh, vh = heads(q.double()) * scale, heads(k.double()), heads(v.double())
    Tk = k.shape[1]
    vis = (torch.arange(Tk)[None, None] < nvis[:, :, None])[:, None]             # [B, 1, Sq, Tk]
    has = vis.any(-1, keepdim=True)
    s = qh @ kh.transpose(-1, -2)
    A = qh.abs() @ kh.abs().transpose(-1, -2)
    m = s.masked_fill(~vis, float("-inf")).amax(-1, keepdim=True)
    w = torch.where(vis & has, torch.exp(s - torch.where(has, m, torch.zeros_like(m))), torch.zeros_like(s))
    w = w / w.sum(-1, keepdim=True).clamp(min=1e-300)
    B, Sq = nvis.shape
    full = lambda x: x.expand(B, HEADS, Sq, 1)
    return dict(ref=w @ vh, S=w @ vh.abs(), A_max=A.masked_fill(~vis, 0.0).amax(-1, keepdim=True),
                spread_max=(m - s).masked_fill(~vis, 0.0).amax(-1, keepdim=True), nvis=full(nvis[:, None, :, None].double()), has_keys=full(has))


class AttnCase:
    """Operands (fp32, CPU) and reference of one (case, family).  q is stored for scale = vd.SCALE; q * vd.SCALE (exact: a power of two)
    with scale 1 is the same product."""

    def __init__(self, name, family):
        self.name, self.family = name, family
        self.B, self.Sq, self.Tk, self.counts, self.causal, self.offset = ATTN_CASES[name]
        self.nvis = visible_counts(self.B, self.Sq, self.Tk, self.counts, self.causal, self.offset)
        self.q, self.k, self.v = attn_values(family, self.B, self.Sq, self.Tk, self.nvis)
        self.r = attn_reference(self.q, self.k, self.v, self.nvis, vd.SCALE)
        self.live = self.nvis.amax(1)  # [B]: rows of k and v below this are read by some query; the rest hold NaN on the device

    def counts_tensor(self):
        return None if self.counts is None else torch.tensor(self.counts, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def attn_case(name, family):
    return AttnCase(name, family)


# ---- pool attention ---------------------------------------------------------------------------------------------------------------------
# name -> (S_max, counts): one query per slot over a k|v cache [slots, S_max, 1536]
POOL_CASES = {
    "mixed": (1030, [1, 256, 257, 600, 0, 63, 64, 65, 255, 512, 513, 1000, 129, 768, 769, 2]),
    "full": (132, [(37 * s) % 131 for s in range(60)] + [0, -1, 130, 1]),  # 64 slots; 37 s mod 131 is 0 at s = 0 too
}
POOL_BOUNDS = (256, 257, 600, 1024)


class PoolCase:
    def __init__(self, name, family, seed=0):
        self.name, self.family, self.causal = "pool-" + name, family, 0
        self.S_max, self.counts = POOL_CASES[name]
        self.slots = len(self.counts)
        self.nvis = torch.tensor(self.counts).clamp(min=0)[:, None]  # [slots, 1]
        Tk = max(int(self.nvis.max()), 1)
        self.Tk = Tk
        q, self.k, self.v = attn_values(family, self.slots, 1, Tk, self.nvis, seed=seed + 5)
        self.q = (q * vd.SCALE).float()  # the pool's attention has scale 1: q arrives scaled
        self.r = attn_reference(self.q, self.k, self.v, self.nvis, 1.0)


@functools.lru_cache(maxsize=None)
def pool_case(name, family, seed=0):
    return PoolCase(name, family, seed)
