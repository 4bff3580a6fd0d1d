"""The text decoder's and the GPT-2 scorer's two fp32 kernels (csrc/decoder.hip: skinny_gemm_kernel; dec_attention_kernel with
dec_attention_combine) pinned per element, in every form a caller launches:

  loco_op_skinny_gemm                 every slicing of skinny_gemm_slices, N around the columns of a workgroup, the three epilogues
  loco_op_skinny_gemm_split           the decode step's two destinations, and the slot pool's ROWS form (destination row per clip from the device)
  loco_op_decoder_attention_strided   packed, the language model's fused q|k|v (ld 2304), the decoder's k|v cache (ld 1536, S_max > Tk rows per clip)
  loco_op_decoder_pool_attention      the slot pool's fixed 256-key splits

Cases, operands and fp64 references are tests/decoder_contract_cases.py's; the bars (a count of roundings read off the kernels, times the
forward-error scale of the element) and the guard machinery are tests/op_check.py's; tests/test_decoder_contract_ref.py shows on the CPU that
an fp32 restatement passes these assertions and that a dropped key, an extra key, a lost k-chunk, a wrong weight row, an off-by-one
causal edge and an unweighted split do not.

Every input sits in a NaN-filled allocation: the gap columns of A, W and R and what lies behind their last rows; the k and v rows that no
query of the clip sees (at or beyond key_counts[b], or beyond the last query's causal edge), the gap columns of q and of the cache, the
scratch of the splits.  Every output sits in a sentinel-filled allocation: each element the operator does not own must keep the sentinel's
bits -- for the ROWS form that includes the cache rows of dropped clips and all rows but (m, c2_rows[m]) -- and each owned element must lose
them.  A query without a visible key yields exactly 0.0.
"""
import ctypes

import pytest
import torch

import decoder_contract_cases as dc
import value_domain_cases as vd

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import op_check as oc
    from gpu_util import check, lib, ptr, stream
    from op_check import Layout, Subset

F32 = torch.float32
HID = 768
NAN = float("nan")


def at(buf, elements=0):
    """pointer to element `elements` of a device tensor"""
    return ctypes.c_void_p(buf.data_ptr() + elements * buf.element_size())


def placed(values, layout):
    """a host matrix (or [nb1, rows, cols] batch) in a NaN-filled device allocation of the layout"""
    return oc.poisoned(values.to("cuda", F32).reshape(layout.nb1, layout.nb2, layout.rows, layout.cols), layout)


def nan_scratch(nbytes):
    return torch.full((nbytes // 4 + 64,), NAN, dtype=F32, device="cuda")


# ---- skinny GEMM ------------------------------------------------------------------------------------------------------------------------
def plain_gemm(a, la_, w, lw_, b, M, N, K):
    """loco_op_skinny_gemm without an epilogue into a dense [M, N]"""
    c = torch.full((M, N), NAN, device="cuda")
    check(lib().loco_op_skinny_gemm(oc.base(a, la_), la_.ld, oc.base(w, lw_), lw_.ld, ptr(b), None, 0, ptr(c), N, M, N, K, 0, stream()), "skinny_gemm")
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("case", dc.GEMM_CASES, ids=dc.gemm_id)
def test_skinny_gemm(case):
    M, N, K, epi, has_bias = case
    A, W, bias, R = dc.gemm_operands(M, N, K)
    la_, lw_, lr_, lc_ = Layout(M, K, ld=K + 8), Layout(N, K, ld=K + 4), Layout(M, N, ld=N + 5), Layout(M, N, ld=N + 7)
    a, w, r = placed(A, la_), placed(W, lw_), placed(R, lr_)
    b = bias.cuda() if has_bias else None
    c = oc.sentinel_buffer(lc_, F32)
    check(lib().loco_op_skinny_gemm(oc.base(a, la_), la_.ld, oc.base(w, lw_), lw_.ld, ptr(b), oc.base(r, lr_) if epi == 2 else None, lr_.ld,
                                    oc.base(c, lc_), lc_.ld, M, N, K, epi, stream()), "skinny_gemm")
    torch.cuda.synchronize()
    oc.assert_guards(c, lc_, f"skinny_gemm {dc.gemm_id(case)}")
    ref, pre, S = oc.reference(A.double(), W.double(), bias.double() if has_bias else None, R.double(), epi)
    bar = oc.element_bar(ref, pre, S, oc.skinny_count(N, K, has_bias, epi == 2), epi)
    oc.assert_elements("decoder_contract.skinny_gemm", oc.owned(c, lc_), ref, S, bar, M=M, N=N, K=K, epilogue=epi, bias=has_bias,
                       slices=oc.skinny_slices(N, K))


SPLIT_N, SPLIT_K = 2304, 768  # the q | k|v product of a decoder layer


def split_operands(M):
    A, W, bias, _ = dc.gemm_operands(M, SPLIT_N, SPLIT_K)
    la_, lw_ = Layout(M, SPLIT_K, ld=SPLIT_K + 8), Layout(SPLIT_N, SPLIT_K, ld=SPLIT_K + 4)
    return placed(A, la_), la_, placed(W, lw_), lw_, bias.cuda()


@pytest.mark.parametrize("M", [5, 64])
@pytest.mark.parametrize("nsplit", [768, 0, SPLIT_N])
def test_skinny_gemm_two_destinations(nsplit, M):
    """The decode step's form: columns [0, nsplit) to C, the rest to C2; each guarded on its own, the values those of the plain operator
    bit for bit (which test_skinny_gemm pins per element at this N and K)."""
    N, K = SPLIT_N, SPLIT_K
    a, la_, w, lw_, b = split_operands(M)
    plain = plain_gemm(a, la_, w, lw_, b, M, N, K)
    l1, l2 = Layout(M, nsplit, ld=nsplit + 7), Layout(M, N - nsplit, ld=N - nsplit + 9)
    c1, c2 = oc.sentinel_buffer(l1, F32), oc.sentinel_buffer(l2, F32)
    check(lib().loco_op_skinny_gemm_split(oc.base(a, la_), la_.ld, oc.base(w, lw_), lw_.ld, ptr(b), oc.base(c1, l1), l1.ld, oc.base(c2, l2), l2.ld,
                                          None, 0, nsplit, M, N, K, stream()), "skinny_gemm_split")
    torch.cuda.synchronize()
    oc.assert_guards(c1, l1, f"split C nsplit={nsplit}")
    oc.assert_guards(c2, l2, f"split C2 nsplit={nsplit}")
    got = torch.cat([oc.owned(c1, l1)[0, 0], oc.owned(c2, l2)[0, 0]], 1).contiguous()
    assert oc.same_bits(got, plain)
    assert not bool(plain.isnan().any())


@pytest.mark.parametrize("nsplit", [768, 0, SPLIT_N])
def test_skinny_gemm_rows(nsplit):
    """The slot pool's form: row m of the C2 part lands in row c2_rows[m] of clip m's cache [M][S_max][width] and nowhere when that is
    negative.  The owned set is exactly the rows (m, c2_rows[m]), columns [0, N - nsplit)."""
    N, K, M, S_max = SPLIT_N, SPLIT_K, 7, 5
    rows = [4, 0, -1, 2, 4, -1, 1]
    width = max(1536, N - nsplit)  # 1536 = the k|v cache's row; the unsplit product needs 2304
    a, la_, w, lw_, b = split_operands(M)
    plain = plain_gemm(a, la_, w, lw_, b, M, N, K)
    l1 = Layout(M, nsplit, ld=nsplit + 7)
    c1 = oc.sentinel_buffer(l1, F32)
    kept = [m for m in range(M) if rows[m] >= 0]
    pos = torch.cat([(m * S_max + rows[m]) * width + torch.arange(N - nsplit) for m in kept])
    span = M * S_max * width
    head = 64
    total = head + span + oc.TILE_SLACK * width
    c2 = torch.full((total,), oc.SENTINEL[F32], dtype=torch.int32, device="cuda").view(F32)
    rows_d = torch.tensor(rows, dtype=torch.int32, device="cuda")
    check(lib().loco_op_skinny_gemm_split(oc.base(a, la_), la_.ld, oc.base(w, lw_), lw_.ld, ptr(b), oc.base(c1, l1), l1.ld, at(c2, head), S_max * width,
                                          ptr(rows_d), width, nsplit, M, N, K, stream()), "skinny_gemm_split rows")
    torch.cuda.synchronize()
    oc.assert_guards(c1, l1, f"rows C nsplit={nsplit}")
    assert oc.same_bits(oc.owned(c1, l1)[0, 0].contiguous(), plain[:, :nsplit].contiguous())
    if nsplit == N:  # nothing goes to C2
        assert int((c2.view(torch.int32) != oc.SENTINEL[F32]).sum()) == 0
        return
    l2 = Subset(pos, span, head=head, tail=oc.TILE_SLACK * width)
    oc.assert_guards(c2, l2, f"rows C2 nsplit={nsplit}")
    got = oc.owned(c2, l2).view(len(kept), N - nsplit)
    assert oc.same_bits(got.contiguous(), plain[kept, nsplit:].contiguous())


# ---- decoder attention ------------------------------------------------------------------------------------------------------------------
def with_dead_rows(x, live):
    """[B, T, C] host tensor with NaN from row live[b] of clip b on"""
    x = x.clone()
    for b in range(x.shape[0]):
        x[b, int(live[b]):] = NAN
    return x


def strided_launch(c, q, ldq, sq, k, ldk, sk, v, ldv, sv, scale, lo):
    """two launches of the strided operator into fresh sentinel buffers of layout lo: guards, the same bits twice; -> out [B, Sq, 768]"""
    nb = int(lib().loco_decoder_attention_scratch_bytes(c.B, c.Sq, c.Tk))
    assert (nb > 0) == (oc.dec_attention_splits(c.B, c.Sq, c.Tk)[0] > 1)
    counts = c.counts_tensor()
    counts = counts.cuda() if counts is not None else None
    outs = []
    for _ in range(2):
        scratch = nan_scratch(nb)
        out = oc.sentinel_buffer(lo, F32)
        check(lib().loco_op_decoder_attention_strided(q, ldq, sq, k, ldk, sk, v, ldv, sv, ptr(counts), oc.base(out, lo), lo.ld, lo.s1, c.B, c.Sq, c.Tk,
                                                      c.causal, c.offset, scale, ptr(scratch), nb, stream()), "decoder_attention_strided")
        torch.cuda.synchronize()
        oc.assert_guards(out, lo, f"attention {c.name} {c.family}")
        outs.append(oc.owned(out, lo)[:, 0].contiguous())
    assert oc.same_bits(outs[0], outs[1]), "two launches differ"
    return outs[0]


def run_packed(c):
    B, Sq, Tk = c.B, c.Sq, c.Tk
    lq, lk, lo = Layout(B * Sq, HID), Layout(B * Tk, HID), Layout(Sq, HID, nb1=B, s1=Sq * HID)
    q = placed(c.q, lq)
    k, v = placed(with_dead_rows(c.k, c.live), lk), placed(with_dead_rows(c.v, c.live), lk)
    out = strided_launch(c, oc.base(q, lq), HID, Sq * HID, oc.base(k, lk), HID, Tk * HID, oc.base(v, lk), HID, Tk * HID, vd.SCALE, lo)
    # the packed operator on the same buffers
    nb = int(lib().loco_decoder_attention_scratch_bytes(B, Sq, Tk))
    scratch = nan_scratch(nb)
    counts = c.counts_tensor()
    counts = counts.cuda() if counts is not None else None
    ref = oc.sentinel_buffer(lo, F32)
    check(lib().loco_op_decoder_attention(oc.base(q, lq), oc.base(k, lk), oc.base(v, lk), ptr(counts), oc.base(ref, lo), B, Sq, Tk, c.causal, c.offset,
                                          vd.SCALE, ptr(scratch), nb, stream()), "decoder_attention")
    torch.cuda.synchronize()
    oc.assert_guards(ref, lo, f"packed operator {c.name}")
    assert oc.same_bits(out, oc.owned(ref, lo)[:, 0].contiguous()), "strided and packed operators differ"
    return out


def run_cache(c):
    """k | v rows of 1536 floats, S_max rows per clip of which Tk may be seen; q arrives scaled (scale 1); every stride wider than its row"""
    B, Sq, Tk = c.B, c.Sq, c.Tk
    S_max = Tk + 3
    lq = Layout(Sq, HID, ld=HID + 4, nb1=B, s1=Sq * (HID + 4) + 4)
    lkv = Layout(S_max, 2 * HID, nb1=B, s1=S_max * 2 * HID)
    lo = Layout(Sq, HID, ld=HID + 8, nb1=B, s1=Sq * (HID + 8) + 24)
    kv = torch.full((B, S_max, 2 * HID), NAN)
    kv[:, :Tk, :HID], kv[:, :Tk, HID:] = c.k, c.v
    q = placed(c.q * vd.SCALE, lq)
    kvd = placed(with_dead_rows(kv, c.live), lkv)
    return strided_launch(c, oc.base(q, lq), lq.ld, lq.s1, oc.base(kvd, lkv), lkv.ld, lkv.s1, at(kvd, lkv.head + HID), lkv.ld, lkv.s1, 1.0, lo)


def run_fused(c):
    """the language model's: q | k | v the columns of one [B, S, 2304] buffer, out rows of 768"""
    B, S = c.B, c.Sq
    assert c.Tk == S
    lf, lo = Layout(S, 3 * HID, nb1=B, s1=S * 3 * HID), Layout(S, HID, nb1=B, s1=S * HID)
    f = placed(torch.cat([c.q, with_dead_rows(c.k, c.live), with_dead_rows(c.v, c.live)], -1), lf)
    p = lambda col: at(f, lf.head + col)
    return strided_launch(c, p(0), lf.ld, lf.s1, p(HID), lf.ld, lf.s1, p(2 * HID), lf.ld, lf.s1, vd.SCALE, lo)


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("name", list(dc.ATTN_CASES))
def test_decoder_attention(name, family):
    c = dc.attn_case(name, family)
    nsplit, _ = oc.dec_attention_splits(c.B, c.Sq, c.Tk)
    layouts = [("packed", run_packed), ("cache", run_cache)] + ([("fused", run_fused)] if name in dc.FUSED_CASES else [])
    for layout, run in layouts:
        out = run(c)
        oc.assert_dec_attention("decoder_contract.attention", dc.heads(out.cpu()), c.r, nsplit, case=name, family=family, layout=layout, splits=nsplit)


# ---- pool attention ---------------------------------------------------------------------------------------------------------------------
class PoolBuffers:
    """q [slots, 768] and the k|v cache [slots, S_max, 1536] of a pool case on the device, dead rows NaN"""

    def __init__(self, S_max, q, k, v, counts):
        self.slots, self.S_max, Tk = q.shape[0], S_max, k.shape[1]
        self.lq, self.lkv = Layout(self.slots, HID), Layout(S_max, 2 * HID, nb1=self.slots, s1=S_max * 2 * HID)
        kv = torch.full((self.slots, S_max, 2 * HID), NAN)
        kv[:, :Tk, :HID], kv[:, :Tk, HID:] = k, v
        self.live = torch.tensor(counts).clamp(min=0)
        self.q, self.kv = placed(q.reshape(self.slots, HID), self.lq), placed(with_dead_rows(kv, self.live), self.lkv)
        self.counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
        self.lo = Layout(self.slots, HID)

    def pool(self, bound):
        nb = int(lib().loco_decoder_pool_attention_scratch_bytes(self.slots, bound))
        scratch = nan_scratch(nb)
        out = oc.sentinel_buffer(self.lo, F32)
        check(lib().loco_op_decoder_pool_attention(oc.base(self.q, self.lq), oc.base(self.kv, self.lkv), self.lkv.ld, self.lkv.s1,
                                                   at(self.kv, self.lkv.head + HID), ptr(self.counts), oc.base(out, self.lo), self.slots, bound,
                                                   ptr(scratch), nb, stream()), "decoder_pool_attention")
        torch.cuda.synchronize()
        oc.assert_guards(out, self.lo, f"pool attention bound {bound}")
        return oc.owned(out, self.lo)[0, 0].contiguous()

    def strided(self, Tk):
        """the strided operator on the same buffers: one query per clip, scale 1"""
        assert oc.dec_attention_splits(self.slots, 1, Tk)[0] == 1
        out = oc.sentinel_buffer(self.lo, F32)
        check(lib().loco_op_decoder_attention_strided(oc.base(self.q, self.lq), HID, HID, oc.base(self.kv, self.lkv), self.lkv.ld, self.lkv.s1,
                                                      at(self.kv, self.lkv.head + HID), self.lkv.ld, self.lkv.s1, ptr(self.counts), oc.base(out, self.lo),
                                                      HID, HID, self.slots, 1, Tk, 0, 0, 1.0, None, 0, stream()), "decoder_attention_strided")
        torch.cuda.synchronize()
        oc.assert_guards(out, self.lo, "strided operator on the pool's buffers")
        return oc.owned(out, self.lo)[0, 0].contiguous()


def pool_buffers(c):
    return PoolBuffers(c.S_max, c.q, c.k, c.v, c.counts)


def same_rows(a, b, rows):
    rows = torch.as_tensor(rows, device=a.device)
    return oc.same_bits(a[rows].contiguous(), b[rows].contiguous())


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("name", list(dc.POOL_CASES))
def test_pool_attention(name, family):
    """Per element at the widest bound; then, slot by slot, the same bits at every bound that covers the slot's count -- its own count
    rounded up to a tile and to a split, 256, 257, 600, 1024 -- and, for counts up to 256, the bits of the strided operator at Tk = 256
    (one split, written directly)."""
    c = dc.pool_case(name, family)
    pb = pool_buffers(c)
    top = max(dc.POOL_BOUNDS)
    canon = pb.pool(top)
    oc.assert_dec_attention("decoder_contract.pool_attention", dc.heads(canon.cpu()[:, None]), c.r, oc.dec_pool_attention_splits(top), case=name,
                            family=family, bound=top)
    live = [max(n, 0) for n in c.counts]
    zero = [s for s in range(pb.slots) if live[s] == 0]
    assert zero and bool((canon[zero] == 0).all())
    own = {-(-n // 64) * 64 for n in live if n > 0} | {-(-n // 256) * 256 for n in live if n > 0}
    compared = 0
    for bound in sorted(set(dc.POOL_BOUNDS) | own):
        covered = [s for s in range(pb.slots) if live[s] <= bound]
        assert same_rows(pb.pool(bound), canon, covered), f"bound {bound}: a covered slot differs from its bits at bound {top}"
        compared += len(covered)
    assert compared > pb.slots * len(dc.POOL_BOUNDS) // 2
    short = [s for s in range(pb.slots) if live[s] <= 256]
    assert same_rows(pb.strided(256), canon, short), "a slot of at most 256 keys differs from the strided operator's single split"


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_pool_attention_ignores_other_slots(family):
    """A slot's output keeps its bits when the other slots' queries, keys, values and counts change"""
    c, other = dc.pool_case("mixed", family), dc.pool_case("mixed", family, 1)
    slots = len(c.counts)
    canon = pool_buffers(c).pool(1024)
    for parity in (0, 1):
        kept = torch.arange(slots) % 2 == parity
        pick = lambda x, y: torch.where(kept.view(-1, *[1] * (x.dim() - 1)), x, y)
        counts = [c.counts[s] if bool(kept[s]) else c.counts[(s + 3) % slots] for s in range(slots)]
        assert any(counts[s] != c.counts[s] for s in range(slots))
        mixed = PoolBuffers(c.S_max, pick(c.q, other.q), pick(c.k, other.k), pick(c.v, other.v), counts)
        out = mixed.pool(1024)
        assert same_rows(out, canon, torch.nonzero(kept).reshape(-1)), "a slot's output moved with its neighbours"
        assert not same_rows(out, canon, torch.nonzero(~kept).reshape(-1))  # the others did change
