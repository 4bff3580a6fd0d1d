"""The bars of the decoder's per-element contract (tests/op_check.py: skinny_count, dec_attention_bar) are neither vacuous nor too tight,
shown on the CPU: a plain fp32 restatement of each operator, in a summation order that is not the kernel's but is as legitimate, passes
the assertions of tests/test_gpu_decoder_contract.py at the same cases; the same restatement with one defect planted misses them, in every
value family.

Restatements.
  skinny GEMM   the kernel's blocking (64 lanes x 4 elements per 256-element chunk, ks slices) in other orders: a lane's chain runs from its
                last chunk and element to its first (fmaf restated as an exact float64 product, one float64 sum, one rounding to fp32), the
                64 lanes meet in a tree over neighbours (1, 2, 4 ... instead of the butterfly's 32, 16 ...), the slices are merged last to first.
  attention     no online softmax and no tiles: per split a two-pass softmax (torch's fp32 max, exp, sum and matmul over the split's whole
                key range), the splits merged last to first with exp(ms - m).  Splits are the launch's own (op_check restates the rules).
Defects.  GEMM: one 256-element k-chunk left out; the last column computed from row N - 2's weights.  Attention: one key dropped at a tile
boundary (the first key of each row's last tile); one extra key past the count (k holds NaN there, as on the device, wherever no query of
the clip sees the row); causal visibility off by one; the partial of the split with the lowest maximum merged without its exp(ms - m) weight.
"""
import pytest
import torch

import decoder_contract_cases as dc
import op_check as oc
import value_domain_cases as vd


# ---- skinny GEMM ------------------------------------------------------------------------------------------------------------------------
def gemm_restated(A, W, bias, R, epi, drop_chunk=None, wrong_last_column=False):
    M, K = A.shape
    N = W.shape[0]
    ks, chunks = oc.skinny_slices(N, K), K // 256
    if wrong_last_column:
        W = W.clone()
        W[N - 1] = W[N - 2]
    A4, W4 = A.view(M, chunks, 64, 4).double(), W.view(N, chunks, 64, 4).double()
    parts = []
    for s in range(ks):
        acc = torch.zeros((M, N, 64), dtype=torch.float32)
        for ch in reversed(range(s, chunks, ks)):
            if ch == drop_chunk:
                continue
            for e in (3, 2, 1, 0):
                acc = (A4[:, None, ch, :, e] * W4[None, :, ch, :, e] + acc.double()).float()
        for _ in range(6):
            acc = acc[..., 0::2] + acc[..., 1::2]
        parts.append(acc[..., 0])
    v = parts[-1]
    for s in reversed(range(ks - 1)):
        v = v + parts[s]
    if bias is not None:
        v = v + bias
    if epi == 1:
        v = torch.nn.functional.gelu(v)
    if epi == 2:
        v = v + R
    return v


def gemm_check(case, out, **tags):
    M, N, K, epi, has_bias = case
    A, W, bias, R = dc.gemm_operands(M, N, K)
    ref, pre, S = oc.reference(A.double(), W.double(), bias.double() if has_bias else None, R.double(), epi)
    bar = oc.element_bar(ref, pre, S, oc.skinny_count(N, K, has_bias, epi == 2), epi)
    return oc.assert_elements("decoder_contract_ref.gemm", out, ref, S, bar, M=M, N=N, K=K, epilogue=epi, **tags)


@pytest.mark.parametrize("case", dc.GEMM_CASES, ids=dc.gemm_id)
def test_gemm_restatement_and_defects(case):
    M, N, K, epi, has_bias = case
    A, W, bias, R = dc.gemm_operands(M, N, K)
    args = (A, W, bias if has_bias else None, R, epi)
    gemm_check(case, gemm_restated(*args))
    with pytest.raises(AssertionError):
        gemm_check(case, gemm_restated(*args, drop_chunk=K // 256 - 1), defect="chunk")
    if N >= 2:
        with pytest.raises(AssertionError):
            gemm_check(case, gemm_restated(*args, wrong_last_column=True), defect="column")


def test_slice_rule():
    """the restated rule at the points the cases were chosen by"""
    s = oc.skinny_slices
    assert [s(81, 256), s(81, 512), s(81, 768), s(128, 1024), s(129, 1024), s(132, 1024), s(81, 1280), s(2304, 1792), s(2304, 2048), s(1, 3072)] == \
        [1, 2, 2, 4, 2, 2, 4, 2, 4, 4]
    assert oc.skinny_count(81, 1280) == 4 * 2 + 6 + 3 + 1 and oc.skinny_count(768, 3072, False, True) == 4 * 3 + 6 + 3 + 1
    assert oc.dec_attention_splits(1, 1, 257) == (2, 192) and oc.dec_attention_splits(7, 1, 600) == (3, 256)
    assert oc.dec_attention_splits(3, 120, 300) == (1, 320) and oc.dec_attention_splits(1, 300, 300) == (2, 192)
    assert [oc.dec_pool_attention_splits(t) for t in (1, 256, 257, 600, 1024)] == [1, 1, 2, 3, 4]


# ---- attention --------------------------------------------------------------------------------------------------------------------------
NINF = torch.tensor(float("-inf"))


def attention_restated(q, k, v, nvis, scale, keys_per_split, nsplit, hidden=None, weightless_split=False):
    """q [B, Sq, 768], k, v [B, Tk, 768] fp32, nvis [B, Sq] -> [B, 12, Sq, 64] fp32.  k may hold NaN in rows that no query sees.
    hidden [B, Sq]: a key index that the query does not see although it is below nvis (the dropped key).  weightless_split: of every
    row, the non-empty split with the lowest maximum is merged with weight 1."""
    qh, kh, vh = dc.heads(q * torch.tensor(scale, dtype=torch.float32)), dc.heads(k), dc.heads(v)
    j = torch.arange(k.shape[1])
    s = qh @ kh.transpose(-1, -2)
    seen = j[None, None] < nvis[:, :, None]
    if hidden is not None:
        seen = seen & (j[None, None] != hidden[:, :, None])
    parts = []
    for sp in range(nsplit):
        vis = (seen & (j >= sp * keys_per_split) & (j < (sp + 1) * keys_per_split))[:, None]
        ms = torch.where(vis, s, NINF).amax(-1, keepdim=True)
        p = torch.where(vis, torch.exp(s - torch.where(ms == NINF, torch.zeros_like(ms), ms)), torch.zeros_like(s))
        parts.append((ms, p.sum(-1, keepdim=True), p @ vh))
    all_ms = torch.stack([ms for ms, _, _ in parts])
    m = all_ms.amax(0)
    lowest = torch.where(all_ms == NINF, -NINF, all_ms).argmin(0)  # per row, the non-empty split with the lowest maximum
    l, o = torch.zeros_like(m), torch.zeros_like(parts[0][2])
    for sp in reversed(range(nsplit)):
        ms, ls, os_ = parts[sp]
        w = torch.where(ms == NINF, torch.zeros_like(ms), torch.exp(ms - torch.where(m == NINF, torch.zeros_like(m), m)))
        if weightless_split:
            w = torch.where((lowest == sp) & (ms > NINF), torch.ones_like(w), w)
        l, o = l + ls * w, o + os_ * w
    return torch.where(l > 0, o / l, torch.zeros_like(o))


def run_attention(tag, c, nsplit, keys_per_split, scale, q):
    """the restatement passes; each defect the case can have misses.  Returns the defects planted."""
    name = "decoder_contract_ref." + tag
    tags = dict(case=c.name, family=c.family)
    B, Sq, Tk = q.shape[0], q.shape[1], c.k.shape[1]
    assert nsplit * keys_per_split > Tk  # the extra key below lies inside the last split
    # k with one more row, NaN from the first row on that no query of the clip sees: what the device buffers of the GPU test hold
    k = torch.cat([c.k, torch.full_like(c.k[:, :1], float("nan"))], 1)
    for b in range(B):
        k[b, int(c.nvis[b].max()):] = float("nan")
    v = torch.cat([c.v, torch.zeros_like(c.v[:, :1])], 1)
    run = lambda nvis, **kw: attention_restated(q, k, v, nvis, scale, keys_per_split, nsplit, **kw)
    n = c.nvis
    oc.assert_dec_attention(name, run(n), c.r, nsplit, **tags)
    defects = {"extra_key": run(n + 1)}
    if bool((n > 0).any()):
        defects["dropped_key"] = run(n, hidden=torch.where(n > 0, 64 * ((n - 1) // 64), -1))  # the first key of the row's last tile
    if c.causal:
        defects["causal_off_by_one"] = run(dc.visible_counts(B, Sq, Tk, c.counts, 1, c.offset + 1))
    if nsplit > 1 and bool((n > keys_per_split).any()):  # a row with keys in split 0 and beyond it
        defects["weightless_split"] = run(n, weightless_split=True)
    for d, out in defects.items():
        with pytest.raises(AssertionError):
            oc.assert_dec_attention(name, out, c.r, nsplit, defect=d, **tags)
    return set(defects)


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("name", list(dc.ATTN_CASES))
def test_attention_restatement_and_defects(name, family):
    c = dc.attn_case(name, family)
    nsplit, kps = oc.dec_attention_splits(c.B, c.Sq, c.Tk)
    planted = run_attention("attention", c, nsplit, kps, vd.SCALE, c.q)
    assert ("causal_off_by_one" in planted) == bool(c.causal)
    if name in ("split2-193", "split2-257", "split3", "causal-cross", "lm-300", "counts-split"):
        assert "weightless_split" in planted and "dropped_key" in planted


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_pool_restatement_and_defects(family):
    c = dc.pool_case("mixed", family)
    planted = run_attention("pool", c, oc.dec_pool_attention_splits(1024), 256, 1.0, c.q)
    assert planted == {"extra_key", "dropped_key", "weightless_split"}


# ---- the operators' argument checks (refused before any launch: no GPU needed) ------------------------------------------------------------
def test_operator_argument_checks():
    import ctypes as C
    import importlib
    lib = importlib.import_module("loco-asr_amd._lib").load()
    buf = (C.c_float * 256)()  # host memory stands in for the pointers
    p = C.cast(buf, C.c_void_p)
    err = lib.loco_last_error
    INVALID, WORKSPACE = -1, -3
    g = lib.loco_op_skinny_gemm_split
    assert g(p, 768, p, 768, None, p, 768, None, 1536, None, 0, 768, 2, 2304, 768, None) == INVALID and b"loco_op_skinny_gemm_split: null" in err()
    assert g(p, 768, p, 768, None, p, 768, p, 1536, None, 0, 768, 65, 2304, 768, None) == INVALID and b"64" in err()
    assert g(p, 768, p, 768, None, p, 768, p, 1536, None, 0, 768, 2, 2304, 700, None) == INVALID and b"256" in err()
    assert g(p, 768, p, 768, None, p, 768, p, 1536, None, 0, 2305, 2, 2304, 768, None) == INVALID and b"nsplit" in err()
    assert g(p, 768, p, 768, None, p, 768, p, 1536, None, 0, -1, 2, 2304, 768, None) == INVALID and b"nsplit" in err()
    assert g(p, 770, p, 768, None, p, 768, p, 1536, None, 0, 768, 2, 2304, 768, None) == INVALID and b"multiples of 4" in err()
    assert g(p, 768, p, 768, None, p, 768, p, 1535, None, 0, 768, 2, 2304, 768, None) == INVALID and b"shorter" in err()
    assert g(p, 768, p, 768, None, p, 768, p, 1 << 20, p, 1535, 768, 2, 2304, 768, None) == INVALID and b"shorter" in err()
    a = lib.loco_op_decoder_attention_strided
    ok = (p, 768, 768, p, 768, 768, p, 768, 768, None, p, 768, 768)
    assert a(*ok, 1, 1, 0, 0, 0, 1.0, None, 0, None) == INVALID and b"loco_op_decoder_attention_strided" in err()
    assert a(None, *ok[1:], 1, 1, 1, 0, 0, 1.0, None, 0, None) == INVALID and b"null" in err()
    assert a(p, 767, *ok[2:], 1, 1, 1, 0, 0, 1.0, None, 0, None) == INVALID and b"768" in err()
    assert a(p, 768, 770, *ok[3:], 1, 1, 1, 0, 0, 1.0, None, 0, None) == INVALID and b"multiples of 4" in err()
    need = lib.loco_decoder_attention_scratch_bytes(1, 1, 600)
    assert need == 12 * 3 * 66 * 4
    assert a(*ok, 1, 1, 600, 0, 0, 1.0, p, need - 1, None) == WORKSPACE and b"scratch" in err()
    assert a(*ok, 1, 1, 600, 0, 0, 1.0, None, need, None) == WORKSPACE
    pb, pa = lib.loco_decoder_pool_attention_scratch_bytes, lib.loco_op_decoder_pool_attention
    assert pb(0, 256) == 0 and pb(3, 0) == 0 and pb(3, 256) == 3 * 12 * 66 * 4 and pb(3, 257) == 2 * pb(3, 256) and pb(64, 1024) == 64 * 12 * 4 * 66 * 4
    assert pa(p, p, 1536, 1536, p, None, p, 3, 256, p, 1 << 20, None) == INVALID and b"loco_op_decoder_pool_attention: null" in err()
    assert pa(p, p, 1536, 1536, p, p, p, 65, 256, p, 1 << 20, None) == INVALID and b"65" in err()
    assert pa(p, p, 1536, 1536, p, p, p, 3, 0, p, 1 << 20, None) == INVALID
    assert pa(p, p, 764, 1536, p, p, p, 3, 256, p, 1 << 20, None) == INVALID and b"768" in err()
    assert pa(p, p, 1536, 1538, p, p, p, 3, 256, p, 1 << 20, None) == INVALID and b"multiples of 4" in err()
    assert pa(p, p, 1536, 1536, p, p, p, 3, 257, p, pb(3, 257) - 1, None) == WORKSPACE and b"scratch" in err()


