"""The f16x3 GEMM family (gemm_f16x3.hip), the fp32 GEMM and what only loco_forward used to reach, pinned per element.

Every case compares a launch with an fp64 reference formed from the operands the kernel really multiplies, element by element
against a derived bar (tests/op_check.py), keeps the whole-tensor bars of tests/test_gpu_ops.py beside it (rel_l2 < 5e-6 for f16x3,
1e-6 for the fp32 kernel), puts the output inside a sentinel-filled allocation that must come back untouched outside what the
operator owns, and feeds NaN wherever the kernel has no business reading a value.  Where the source promises identical bits
(every tile form, persistent or not; the positional conv's single-pass forms; a residual given as planes or as their fp32 sum;
power-of-two weight scaling) the bits are compared.

Which cases of matrix A.1 take the PERSISTENT branch (launch_tile: fewer than 13 waves, more tiles than workgroup slots, and
K / 32 >= the A ring's depth).  M = 200, N = 520, 13 x 4 problems:
  form  tile      waves  slots  A ring  tiles  K = 64 (2 k-tiles)  K = 160 (5 k-tiles)
  1     256x256   16     -      3       156    no (16 waves)       no
  2     256x128   8      256    3       260    no (ring 3 > 2)     persistent
  3     192x128   6      512    2       520    persistent          persistent
  4     128x128   4      512    2       520    persistent          persistent
  5     128x128   4      256    3       520    no (ring 3 > 2)     persistent
  6     192x256   12     256    3       312    no (ring 3 > 2)     persistent
  7     256x256   16     -      2       156    no (16 waves)       no
  8     128x128   4      256    5       520    no (ring 5 > 2)     persistent (ring 5 = 5)
  auto: K = 64 -> form 4 (K <= 128 and >= 1024 rows), K = 160 -> form 2 (the cost model; N % 256 != 0 leaves forms 2 and 5).
The unbatched ragged cases (449 x 332: at most 12 tiles) and everything in matrix B never go persistent.
"""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import op_check as oc
    from gpu_util import _libmod, check, la, lib, ptr, stream
    from op_check import Layout, knobs

F16, F32 = torch.float16, torch.float32
FORMS = (0, 1, 2, 3, 4, 5, 6, 7, 8)  # 0 = the launcher's own choice


def rnd(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).cuda()


def f64(hi, lo=None):
    x = hi.double().cpu()
    return x if lo is None else x + lo.double().cpu()


class Problem:
    """One set of f16x3 operands in padded, NaN-poisoned allocations, with the fp64 products its references share."""

    def __init__(self, seed, M, N, K, nb1=1, nb2=1, pad=True, w_scale=None, out_scale=1.0):
        self.M, self.N, self.K, self.nb1, self.nb2, self.out_scale = M, N, K, nb1, nb2, out_scale
        lda, ldw, ldc = (K + 8, K + 16, N + 8) if pad else (K, K, N)
        sA2, sC2 = (M * lda + 8, M * ldc + 8) if nb1 * nb2 > 1 else (0, 0)
        sA1, sC1 = (nb2 * sA2 + 16, nb2 * sC2 + 16) if nb1 * nb2 > 1 else (0, 0)
        # behind a batched allocation: the usual tile of slack plus what a decode that confused the two batch strides would reach
        tail = lambda ld, s1, s2: oc.TILE_SLACK * (ld + 1) + (nb2 - 1) * (s1 - s2)
        self.la, self.lw = Layout(M, K, lda, nb1, nb2, sA1, sA2, tail=tail(lda, sA1, sA2)), Layout(N, K, ldw)
        self.lc = Layout(M, N, ldc, nb1, nb2, sC1, sC2, tail=tail(ldc, sC1, sC2))
        # plane outputs leave as 16-byte pieces: their row stride is a multiple of 8 halves (N = 332: 344 where the fp32 output has 340)
        self.lcp = self.lc if ldc % 8 == 0 else Layout(M, N, ldc + 4)
        assert nb1 * nb2 == 1 or self.lcp is self.lc
        A = rnd(seed, (nb1, nb2, M, K), 2.0)
        W = rnd(seed + 1, (1, 1, N, K), w_scale if w_scale is not None else 2.0 / math.sqrt(K))
        self.bias = rnd(seed + 2, (N,))
        R = rnd(seed + 3, (nb1, nb2, M, N))
        ahi, alo = oc.split_planes(A)
        whi, wlo = oc.split_planes(W)
        self.set_weights(whi, wlo)
        self.ahi, self.alo = oc.poisoned(ahi, self.la), oc.poisoned(alo, self.la)
        self.R = oc.poisoned(R, self.lc)
        self.a64, self.bias64, self.R64 = f64(ahi, alo), f64(self.bias), f64(R)
        self._prod = {}

    def set_weights(self, whi, wlo):
        self.whi_dense, self.wlo_dense = whi, wlo
        self.whi, self.wlo = oc.poisoned(whi, self.lw), oc.poisoned(wlo, self.lw)
        self._prod = {}

    def prod(self, terms=3):
        """the fp64 products (a w^T, |a| |w|^T) [nb1, nb2, M, N]: formed once per `terms`, shared by every reference, never modified"""
        if terms not in self._prod:
            w64 = f64(self.whi_dense, self.wlo_dense if terms == 3 else None)[0, 0]
            self._prod[terms] = oc.products(self.a64, w64, self.out_scale)
        return self._prod[terms]

    def reference(self, epi, terms=3, R64=None):
        """(ref, pre, S) [nb1, nb2, M, N]"""
        return oc.reference(None, None, self.bias64, self.R64 if R64 is None else R64, epi, prod=self.prod(terms))

    def layout(self, planes):
        return self.lcp if planes else self.lc

    def outputs(self, planes, layout=None):
        lc = layout or self.layout(planes)
        return [oc.sentinel_buffer(lc, F16), oc.sentinel_buffer(lc, F16)] if planes else [oc.sentinel_buffer(lc, F32)]

    def launch(self, epi, planes, splitk=None):
        """loco_op_gemm_f16x3 (or _splitk with a workspace) into fresh guarded outputs"""
        outs = self.outputs(planes)
        a, w, c = self.la, self.lw, self.layout(planes)
        C_, chi, clo = (None, oc.base(outs[0], c), oc.base(outs[1], c)) if planes else (oc.base(outs[0], c), None, None)
        head = (oc.base(self.ahi, a), oc.base(self.alo, a), a.ld, oc.base(self.whi, w), oc.base(self.wlo, w), w.ld, ptr(self.bias),
                oc.base(self.R, self.lc) if epi == 2 else None, self.lc.ld, C_, chi, clo, c.ld, self.M, self.N, self.K, epi)
        if splitk is None:
            check(lib().loco_op_gemm_f16x3(*head, self.nb1, self.nb2, a.s1, a.s2, c.s1, c.s2, stream()))
        else:
            check(lib().loco_op_gemm_f16x3_splitk(*head, ptr(splitk), splitk.numel() * 4, stream()))
        torch.cuda.synchronize()
        return outs

    def verify(self, name, outs, epi, planes, terms=3, layout=None, ref=None, **tags):
        lc = layout or self.layout(planes)
        for o in outs:
            oc.assert_guards(o, lc, f"{name} {tags}")
        ref, pre, S = ref or self.reference(epi, terms)
        out = oc.owned(outs[0], lc).double() + oc.owned(outs[1], lc).double() if planes else oc.owned(outs[0], lc)
        bar = oc.element_bar(ref, pre, S, oc.f16x3_count(self.K, terms), epi, planes)
        return oc.assert_elements(name, out, ref, S, bar, rel_l2_bar=5e-6, M=self.M, N=self.N, K=self.K, epi=epi, planes=planes, **tags)


def assert_same(outs, first, what):
    for o, f in zip(outs, first):
        assert oc.same_bits(o, f), f"{what}: bits differ"


@functools.lru_cache(maxsize=None)
def batched_problem(K):
    return Problem(100 + K, 200, 520, K, nb1=13, nb2=4)


@functools.lru_cache(maxsize=None)
def ragged_problem(K):
    return Problem(200 + K, 449, 332, K)


@functools.lru_cache(maxsize=None)
def splitk_ws():
    """twice what the library asks for: the partial sums of the positional conv are [clip][slice][group][frame][48], and a decode that
    confused their two batch strides would reach 47 MB into it at B = 2, T = 513 -- still inside"""
    return torch.empty(2 * lib().loco_gemm_splitk_bytes() // 4, device="cuda")


# ---- A.1: every tile form, batched + strided, ragged column tail ---------------------------------------------------------------
def every_form(p, name, epi, planes):
    first = None
    for form in FORMS:
        for nopersist in (None, "1"):
            with knobs(LOCO_GEMM_TILE=form or None, LOCO_GEMM_NOPERSIST=nopersist):
                outs = p.launch(epi, planes)
            for o in outs:
                oc.assert_guards(o, p.layout(planes), f"{name} form {form} nopersist {nopersist}")
            if first is None:
                first = outs
                p.verify(name, outs, epi, planes)  # forms 1-8 are held to the same bits below: one figure covers them all
            else:
                assert_same(outs, first, f"{name} form {form} nopersist {nopersist} against the automatic form")


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("K", [64, 160])
def test_f16x3_batched_strided_every_form(K, epi, planes):
    """13 x 4 problems of 200 x 520 with gaps between rows and batch entries: the tile decode (z1, z2, coff, XCD runs, column groups),
    the persistent walk (table in the module docstring) and the 8-column tail of the wide store, in all eight forms, each with and
    without LOCO_GEMM_NOPERSIST, all to the same bits."""
    every_form(batched_problem(K), "f16x3_batched", epi, planes)


@pytest.mark.parametrize("epi,planes", [(0, False), (1, True), (2, True)])
@pytest.mark.parametrize("K", [32, 96, 192])
def test_f16x3_unbatched_ragged_every_form(K, epi, planes):
    """449 x 332 (332 = 12 mod 16; row tiles 128 x 3 + 65, 192 x 2 + 65, 256 + 193), k-loops shorter and longer than every ring"""
    every_form(ragged_problem(K), "f16x3_ragged", epi, planes)


# ---- A.2: split-K -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("M,N", [(1, 332), (130, 332), (1, 768), (130, 768)])
def test_f16x3_splitk(M, N, epi, planes):
    p = _splitk_problem(M, N)
    outs = p.launch(epi, planes, splitk=splitk_ws())
    p.verify("f16x3_splitk", outs, epi, planes)
    assert_same(p.launch(epi, planes, splitk=splitk_ws()), outs, "split-K repeat")


@functools.lru_cache(maxsize=None)
def _splitk_problem(M, N):
    return Problem(300 + M + N, M, N, 768)


# ---- A.3: the fp32 kernel -----------------------------------------------------------------------------------------------------
def gemm_f32(A, la_, W, lw, bias, R, C_, lc, M, N, K, epi):
    check(lib().loco_op_gemm(oc.base(A, la_), la_.ld, oc.base(W, lw), lw.ld, ptr(bias), oc.base(R, lc) if R is not None else None, lc.ld,
                             oc.base(C_, lc), lc.ld, M, N, K, epi, la_.nb1, la_.nb2, la_.s1, la_.s2, lc.s1, lc.s2, stream()))
    torch.cuda.synchronize()


def verify_f32(name, C_, lc, ref, pre, S, K, epi, **tags):
    oc.assert_guards(C_, lc, name)
    bar = oc.element_bar(ref, pre, S, oc.f32_count(K), epi)
    oc.assert_elements(name, oc.owned(C_, lc), ref, S, bar, rel_l2_bar=1e-6, K=K, epi=epi, **tags)


def test_gemm_f32_qp_table_layout():
    """encoder_f32's Qp GEMM: A = the q columns of a [B, T, 2304] q|k|v buffer (head h at column 64 h, lda = 2304), output [B, 12, T, 320].
    The k and v columns hold NaN."""
    B, T, N, K = 2, 130, 320, 64
    la_ = Layout(T, K, 2304, B, 12, T * 2304, 64)
    lw, lc = Layout(N, K), Layout(T, N, N, B, 12, 12 * T * N, T * N)
    q, W = rnd(1, (B, 12, T, K), 0.25), rnd(2, (1, 1, N, K), 1.0)
    C_ = oc.sentinel_buffer(lc, F32)
    gemm_f32(oc.poisoned(q, la_), la_, oc.poisoned(W, lw), lw, None, None, C_, lc, T, N, K, 0)
    ref, pre, S = oc.reference(f64(q), f64(W)[0, 0])
    verify_f32("gemm_f32_qp", C_, lc, ref, pre, S, K, 0, M=T, N=N)


@pytest.mark.parametrize("epi", [0, 1, 2, 5])
def test_gemm_f32_padded(epi):
    M, N, K = 200, 332, 96
    la_, lw, lc = Layout(M, K, K + 4), Layout(N, K), Layout(M, N, N + 4)
    A, W, bias, R = rnd(3, (1, 1, M, K), 2.0), rnd(4, (1, 1, N, K), 2.0 / math.sqrt(K)), rnd(5, (N,)), rnd(6, (1, 1, M, N))
    C_ = oc.sentinel_buffer(lc, F32)
    gemm_f32(oc.poisoned(A, la_), la_, oc.poisoned(W, lw), lw, bias, oc.poisoned(R, lc) if epi == 2 else None, C_, lc, M, N, K, epi)
    ref, pre, S = oc.reference(f64(A), f64(W)[0, 0], f64(bias), f64(R), epi)
    verify_f32("gemm_f32_padded", C_, lc, ref, pre, S, K, epi, M=M, N=N)


# ---- A.4: plane outputs leave as 16-byte pieces ------------------------------------------------------------------------------
@pytest.mark.parametrize("ldc,sC1,sC2", [(132, 0, 0), (136, 0, 64 * 136 + 4), (136, 2 * 64 * 136 + 12, 64 * 136)])
def test_f16x3_plane_output_needs_8_half_strides(ldc, sC1, sC2):
    """ldc, sC1 or sC2 = 4 mod 8 with a plane output: rejected before any launch (an fp32 output accepts multiples of 4)"""
    M, N, K = 64, 128, 32
    z = torch.zeros(2 * 2 * M * 136 + 64, dtype=F16, device="cuda")
    nb = 2 if (sC1 or sC2) else 1
    with pytest.raises(ValueError, match="plane output"):
        check(lib().loco_op_gemm_f16x3(ptr(z), ptr(z), K, ptr(z), ptr(z), K, None, None, 0, None, ptr(z), ptr(z), ldc, M, N, K, 0, nb if sC1 else 1,
                                       nb if sC2 else 1, 0, 0, sC1, sC2, stream()))
    if not sC1 and not sC2:
        with pytest.raises(ValueError, match="plane output"):
            check(lib().loco_op_gemm_f16x3_splitk(ptr(z), ptr(z), K, ptr(z), ptr(z), K, None, None, 0, None, ptr(z), ptr(z), ldc, M, N, K, 0,
                                                  ptr(splitk_ws()), splitk_ws().numel() * 4, stream()))
        with pytest.raises(ValueError, match="plane output"):
            desc_launch(M=M, N=N, K=K, Ahi=ptr(z), Alo=ptr(z), Whi=ptr(z), Wlo=ptr(z), Chi=ptr(z), Clo=ptr(z), lda=K, ldw=K, ldc=ldc)


# ---- B.1: everything loco_forward passes, through loco_op_gemm_f16x3_desc ---------------------------------------------------------
def desc_launch(**kw):
    d = _libmod.LocoGemmF16Desc()
    d.struct_size = C.sizeof(d)
    d.nb1 = d.nb2 = 1
    d.terms, d.out_scale = 3, 1.0
    for k, v in kw.items():
        setattr(d, k, v.value if isinstance(v, C.c_void_p) else v)
    check(lib().loco_op_gemm_f16x3_desc(C.byref(d), stream()))
    torch.cuda.synchronize()


def desc_operands(p):
    a, w = p.la, p.lw
    return dict(M=p.M, N=p.N, K=p.K, Ahi=oc.base(p.ahi, a), Alo=oc.base(p.alo, a), Whi=oc.base(p.whi, w), Wlo=oc.base(p.wlo, w), lda=a.ld,
                ldw=w.ld, bias=ptr(p.bias), out_scale=p.out_scale)


def test_desc_rejects_a_wrong_struct_size():
    d = _libmod.LocoGemmF16Desc()
    d.struct_size = C.sizeof(d) - 8
    with pytest.raises(ValueError, match="struct_size"):
        check(lib().loco_op_gemm_f16x3_desc(C.byref(d), stream()))


def slot_max(slot):
    return float(slot.max())


def plane_absmax(outs, lc):
    return float((oc.owned(outs[0], lc).double() + oc.owned(outs[1], lc).double()).abs().max())


@functools.lru_cache(maxsize=None)
def qkv_problem(M):
    return Problem(400 + M, M, 2304, 768)


@pytest.mark.parametrize("M", [1, 130, 449])
def test_qkv_scatter_every_form_and_splitk(M):
    """kEpiQkvScatter: columns [768 j, 768 j + 768) land in plane pair j, qkv_stride halves apart with guard between the pairs; single
    pass in every tile form (same bits) and through splitk_reduce_qkv_kernel; the range word follows what was written."""
    p = qkv_problem(M)
    stride = 2 * M * 768 + 64
    lq = Layout(M, 768, 768, 1, 3, 0, stride)
    ref, pre, S = p.reference(0)
    scat = lambda x: x.view(M, 3, 768).permute(1, 0, 2).reshape(1, 3, M, 768)
    ref3 = (scat(ref), scat(pre), scat(S))

    def run(ws):
        outs = p.outputs(True, lq)
        slot = torch.zeros(8, device="cuda")
        desc_launch(**desc_operands(p), epilogue=3, Chi=oc.base(outs[0], lq), Clo=oc.base(outs[1], lq), ldc=768, qkv_stride=stride,
                    range_slot=ptr(slot), splitk_ws=ptr(ws), splitk_bytes=ws.numel() * 4 if ws is not None else 0)
        return outs, slot

    first = None
    for form in FORMS:
        with knobs(LOCO_GEMM_TILE=form or None):
            outs, slot = run(None)
        for o in outs:
            oc.assert_guards(o, lq, f"qkv scatter form {form}")
        if first is None:
            first = outs
            p.verify("f16x3_qkv_scatter", outs, 3, True, layout=lq, ref=ref3, path="single pass")
        else:
            assert_same(outs, first, f"qkv scatter form {form}")
        amax = plane_absmax(outs, lq)
        assert abs(slot_max(slot) - amax) <= 2.0 ** -21 * amax, (form, slot_max(slot), amax)
    outs, slot = run(splitk_ws())
    p.verify("f16x3_qkv_scatter", outs, 3, True, layout=lq, ref=ref3, path="split-K")
    amax = plane_absmax(outs, lq)
    assert abs(slot_max(slot) - amax) <= 2.0 ** -21 * amax, (slot_max(slot), amax)
    assert_same(run(splitk_ws())[0], outs, "qkv scatter split-K repeat")


@pytest.mark.parametrize("path", ["single pass", "split-K"])
def test_range_slot_only_grows(path):
    """a word that already holds more than anything written stays as it is (GELU planes; both paths)"""
    p = _splitk_problem(130, 768)
    ws = splitk_ws() if path == "split-K" else None
    outs = p.outputs(True)
    slot = torch.full((8,), 1.0e6, device="cuda")
    desc_launch(**desc_operands(p), epilogue=1, Chi=oc.base(outs[0], p.lc), Clo=oc.base(outs[1], p.lc), ldc=p.lc.ld, range_slot=ptr(slot),
                splitk_ws=ptr(ws), splitk_bytes=ws.numel() * 4 if ws is not None else 0)
    assert bool((slot == 1.0e6).all())
    slot.zero_()
    again = p.outputs(True)
    desc_launch(**desc_operands(p), epilogue=1, Chi=oc.base(again[0], p.lc), Clo=oc.base(again[1], p.lc), ldc=p.lc.ld, range_slot=ptr(slot),
                splitk_ws=ptr(ws), splitk_bytes=ws.numel() * 4 if ws is not None else 0)
    assert_same(again, outs, "range tracking changed the result")
    amax = plane_absmax(outs, p.lc)
    assert abs(slot_max(slot) - amax) <= 2.0 ** -21 * amax, (slot_max(slot), amax)
    p.verify("f16x3_range_slot", outs, 1, True, path=path)


@functools.lru_cache(maxsize=None)
def residual_problem(M, K):
    return Problem(500 + M + K, M, 768, K)


@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("M", [1, 130, 449])
def test_residual_from_planes_equals_residual_from_their_sum(M, K):
    """kEpiResidual with Rhi / Rlo (ldr = 776): the same bits as the call given R = float(Rhi) + float(Rlo), which is exact; R itself
    points at other numbers while the planes are given.  Single pass and split-K."""
    p = residual_problem(M, K)
    lc = p.lc  # ldc = ldr = 776
    assert lc.ld == 776
    rhi, rlo = oc.split_planes(oc.owned(p.R, lc))
    rsum = oc.poisoned(rhi.float() + rlo.float(), lc)
    decoy = oc.poisoned(rnd(9, (1, 1, M, 768)), lc)
    rhi_b, rlo_b = oc.poisoned(rhi, lc), oc.poisoned(rlo, lc)
    ref = p.reference(2, R64=f64(rhi, rlo))
    for ws in (None, splitk_ws()):
        wsa = dict(splitk_ws=ptr(ws), splitk_bytes=ws.numel() * 4 if ws is not None else 0)
        from_planes, from_sum = p.outputs(False), p.outputs(False)
        desc_launch(**desc_operands(p), epilogue=2, C=oc.base(from_planes[0], lc), ldc=lc.ld, ldr=lc.ld, Rhi=oc.base(rhi_b, lc),
                    Rlo=oc.base(rlo_b, lc), R=oc.base(decoy, lc), **wsa)
        desc_launch(**desc_operands(p), epilogue=2, C=oc.base(from_sum[0], lc), ldc=lc.ld, ldr=lc.ld, R=oc.base(rsum, lc), **wsa)
        path = "single pass" if ws is None else "split-K"
        p.verify("f16x3_residual_planes", from_planes, 2, False, ref=ref, path=path)
        assert_same(from_planes, from_sum, f"residual planes against their fp32 sum, {path}")


@pytest.mark.parametrize("M", [1, 130, 449])
def test_out_scale_with_power_of_two_weight_planes(M):
    """Weight planes holding W 2^9 (largest element in [2^13, 2^14), as make_split leaves them) with out_scale = 2^-9 against the
    same planes times 2^-9 with out_scale = 1: identical bits -- the scaling is exact while nothing leaves fp16's normal range, so
    the plane elements below 2^-5 (whose 2^-9 multiple would be subnormal) are set to zero first.  Single pass, split-K and the
    q|k|v reduction (splitk_reduce_qkv_kernel has its own out_scale multiply)."""
    for N, epi in ((768, 1), (2304, 3)):
        p = Problem(600 + M + N, M, N, 768, w_scale=24.0)
        whi, wlo = p.whi_dense.clone(), p.wlo_dense.clone()
        assert 2.0 ** 13 <= float(whi.abs().max()) * 512 < 2.0 ** 14
        up = lambda x: (x.float() * 512).half()
        big_hi, big_lo = up(whi), up(wlo)
        big_hi[big_hi.abs() < 2.0 ** -5] = 0
        big_lo[big_lo.abs() < 2.0 ** -5] = 0
        small_hi, small_lo = (big_hi.float() / 512).half(), (big_lo.float() / 512).half()
        assert oc.same_bits(up(small_hi), big_hi) and oc.same_bits(up(small_lo), big_lo) and bool(torch.isfinite(big_hi).all())
        stride = 2 * M * 768 + 64
        lc = Layout(M, 768, 768, 1, 3, 0, stride) if epi == 3 else p.lc
        ref = None
        for ws in (None, splitk_ws()):
            res = []
            for hi, lo, scale in ((small_hi, small_lo, 1.0), (big_hi, big_lo, 2.0 ** -9)):
                p.set_weights(hi, lo)
                p.out_scale = scale
                outs = p.outputs(True, lc)
                desc_launch(**desc_operands(p), epilogue=epi, Chi=oc.base(outs[0], lc), Clo=oc.base(outs[1], lc), ldc=lc.ld,
                            qkv_stride=stride if epi == 3 else 0, splitk_ws=ptr(ws), splitk_bytes=ws.numel() * 4 if ws is not None else 0)
                res.append(outs)
            path = "single pass" if ws is None else "split-K"
            assert_same(res[1], res[0], f"out_scale 2^-9, N {N}, {path}")
            if ref is None:
                ref = p.reference(1 if epi == 1 else 0)  # of the scaled planes with out_scale = 2^-9, the last ones set
                if epi == 3:
                    ref = tuple(x.view(M, 3, 768).permute(1, 0, 2).reshape(1, 3, M, 768) for x in ref)
            p.verify("f16x3_out_scale", res[1], epi, True, layout=lc, ref=ref, path=path)


@pytest.mark.parametrize("M", [1, 130, 449])
def test_two_term_mode_never_reads_the_weights_lo_plane(M):
    """terms = 2 (precision mode "f16x2"): (Ahi + Alo) Whi with two MFMAs per k-tile, in the five forms the mode has; the Wlo plane
    handed over is NaN throughout."""
    p = residual_problem(M, 768)
    nan_lo = torch.full_like(p.wlo, float("nan"))
    ops = dict(desc_operands(p), Wlo=oc.base(nan_lo, p.lw), terms=2)
    first = None
    for form in (0, 1, 2, 4, 5, 6):
        with knobs(LOCO_GEMM_TILE=form or None):
            outs = p.outputs(False)
            desc_launch(**ops, epilogue=0, C=oc.base(outs[0], p.lc), ldc=p.lc.ld)
        if first is None:
            first = outs
            p.verify("f16x3_two_terms", outs, 0, False, terms=2)
        else:
            oc.assert_guards(outs[0], p.lc, f"terms 2 form {form}")
            assert_same(outs, first, f"terms 2 form {form}")


# ---- B.2: the grouped positional conv on the f16x3 kernels -----------------------------------------------------------------------
POS_CASES = [(1, 1, None, None), (2, 49, [49, 30], None), (3, 129, [129, 1, 77], [129, 40, 129]), (1, 257, None, None),
             (2, 513, [513, 300], None)]


@functools.lru_cache(maxsize=None)
def pos_weights():
    """folded weight [768][48][128] (out, in, tap) -> GEMM order [g][o][tap * 48 + i], times 2^k as make_split scales it, split"""
    import speecht5_oracle as oracle
    sd = la.synth.encoder_state_dict(0, layers=0)
    w = oracle.pos_conv_weight(sd).float()
    wg = w.view(16, 48, 48, 128).permute(0, 1, 3, 2).reshape(16, 48, 6144).contiguous().cuda()
    k = 14 - math.frexp(float(wg.abs().max()))[1]
    whi, wlo = oc.split_planes(wg * 2.0 ** k)
    assert 2.0 ** 13 <= float(whi.abs().max()) < 2.0 ** 14
    bias = torch.from_numpy(sd["prenet.pos_conv_embed.conv.bias"]).cuda()
    return whi, wlo, 2.0 ** -k, bias, f64(whi, wlo) * 2.0 ** -k


class PosRun:
    def __init__(self, h, frames, rows_clip):
        self.B, self.T = h.shape[:2]
        self.h, self.frames, self.rows_clip = h, frames, rows_clip
        # (clip, group) blocks of the scratch are (T + 128) x 48 halves apart and 16 of them per clip; the output's groups are 48
        # columns apart and its clips T x 768: the slack behind each covers a decode that took one stride for the other
        B, T = self.B, self.T
        self.lg = Layout(B * 16 * (T + 128), 48, tail=oc.TILE_SLACK * 49 + 15 * 16 * (T + 128) * 48)
        self.lo_ = Layout(B * T, 768, tail=oc.TILE_SLACK * 769 + 15 * T * 768)
        self.tab = la.sinusoid_table(self.T + 2).cuda()

    def launch(self, ws=None):
        whi, wlo, inv, bias, _ = pos_weights()
        self.ghi, self.glo = oc.sentinel_buffer(self.lg, F16), oc.sentinel_buffer(self.lg, F16)
        out = oc.sentinel_buffer(self.lo_, F32)
        check(lib().loco_op_pos_conv_f16x3(ptr(self.h), ptr(whi), ptr(wlo), ptr(bias), ptr(self.tab), ptr(self.frames), ptr(self.rows_clip), inv, 3,
                                           oc.base(self.ghi, self.lg), oc.base(self.glo, self.lg), ptr(ws), ws.numel() * 4 if ws is not None else 0,
                                           oc.base(out, self.lo_), self.B, self.T, stream()))
        torch.cuda.synchronize()
        for b_, l_ in ((self.ghi, self.lg), (self.glo, self.lg), (out, self.lo_)):
            oc.assert_guards(b_, l_, "positional conv")
        return out

    def check_scratch(self):
        """the group-major planes: fp16 hi / lo of h where t < rows_clip[b], zeros in the 64-frame halo on both sides and beyond the clip"""
        B, T = self.B, self.T
        hi = oc.owned(self.ghi, self.lg).view(B, 16, T + 128, 48)
        lo = oc.owned(self.glo, self.lg).view(B, 16, T + 128, 48)
        x = self.h.view(B, T, 16, 48).permute(0, 2, 1, 3).clone()
        if self.rows_clip is not None:
            x = torch.where(torch.arange(T, device="cuda")[None, None, :, None] < self.rows_clip.long()[:, None, None, None], x, torch.zeros_like(x))
        want = torch.zeros(B, 16, T + 128, 48, device="cuda")
        want[:, :, 64:64 + T] = x
        assert oc.same_bits(hi.contiguous(), want.half()) and oc.same_bits(lo.contiguous(), (want - want.half().float()).half())
        assert not bool(hi[:, :, :64].any()) and not bool(hi[:, :, 64 + T:].any()) and not bool(lo[:, :, :64].any()) and not bool(lo[:, :, 64 + T:].any())
        return f64(hi, lo)

    def verify(self, out, a64, path):
        """fp64 grouped conv of the planes' hi + lo with the weight planes' hi + lo: per (clip, group) the GEMM of the [T, 128 x 48]
        window matrix (row t = padded rows t .. t + 127, a strided view) with the group's [48, 6144] weight"""
        B, T = self.B, self.T
        w64, bias64 = pos_weights()[4], f64(pos_weights()[3])
        a64 = a64.contiguous()
        per_clip = [oc.products(a64[b].as_strided((16, T, 6144), ((T + 128) * 48, 48, 1)), w64) for b in range(B)]  # each [16, T, 48]
        conv, S = torch.stack([c for c, _ in per_clip]), torch.stack([s_ for _, s_ in per_clip])
        conv = conv + bias64.view(1, 16, 1, 48)
        S = S + bias64.abs().view(1, 16, 1, 48)  # the conv's own scale: what GELU's argument is held to
        to_btc = lambda x: x.permute(0, 2, 1, 3).reshape(B * T, 768)
        conv, S = to_btc(conv), to_btc(S)
        g = oc.gelu64(conv)
        fr = self.frames.cpu().long() if self.frames is not None else torch.full((B,), T)
        valid = (torch.arange(T)[None] < fr[:, None]).long()
        pos = torch.cumsum(valid, 1) * valid + 1
        h64, tab64 = f64(self.h).reshape(B * T, 768), f64(self.tab)[pos].reshape(B * T, 768)
        ref = h64 + g + tab64
        # the conv's bar through GELU, plus the two adds of the residual and the sinusoid (one rounding each of at most u times the sum)
        bar = oc.element_bar(g, conv, S, oc.f16x3_count(6144), 1) + 2 * oc.U * (h64.abs() + g.abs() + tab64.abs())
        # recorded against S of the whole expression: conv + bias, the residual h and the sinusoid
        oc.assert_elements("posconv_f16x3", oc.owned(out, self.lo_), ref, S + h64.abs() + tab64.abs(), bar, rel_l2_bar=5e-6, B=B, T=T, path=path)


@pytest.mark.parametrize("B,T,frames,rows_clip", POS_CASES)
def test_pos_conv_f16x3_every_form(B, T, frames, rows_clip):
    """pos_conv_resident_kernel with 256- and 512-frame tiles and the generic 8 x 1 form: the same bits; the 8-slice split-K form: the
    fp64 bar, repeatable, and clip 0's result the same alone as inside the batch; LOCO_GEMM_NOSPLITK takes the workspace away again."""
    h = rnd(700 + T, (B, T, 768), 1.5)
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device="cuda")
    rc = None if rows_clip is None else torch.tensor(rows_clip, dtype=torch.int32, device="cuda")
    r = PosRun(h, fr, rc)
    first = None
    for name, env, ws in (("automatic", {}, None), ("NI=2", dict(LOCO_POSCONV_NI="2"), None), ("NI=4", dict(LOCO_POSCONV_NI="4"), None),
                          ("generic", dict(LOCO_POSCONV_GENERIC="1"), None), ("NOSPLITK", dict(LOCO_GEMM_NOSPLITK="1"), splitk_ws())):
        with knobs(**env):
            out = r.launch(ws)
        if first is None:
            first = out
            a64 = r.check_scratch()
            r.verify(out, a64, "single pass")
        else:
            assert oc.same_bits(out, first), f"positional conv form {name}: bits differ from the automatic form"
    out = r.launch(splitk_ws())
    r.verify(out, a64, "split-K")
    assert oc.same_bits(r.launch(splitk_ws()), out), "positional conv split-K repeat"
    if B > 1:
        alone = PosRun(h[:1].contiguous(), None if fr is None else fr[:1].contiguous(), None if rc is None else rc[:1].contiguous())
        o1 = alone.launch(splitk_ws())
        assert oc.same_bits(oc.owned(o1, alone.lo_), oc.owned(out, r.lo_)[:, :, :T].contiguous()), "split-K: clip 0 depends on its batch"


# ---- B.3: LayerNorm writing planes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [512, 768])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_layernorm_planes_and_nonfinite_slot(rows, dim):
    import torch.nn.functional as F
    x = rnd(800 + rows + dim, (rows, dim), 3.0) + 0.5
    g, b = rnd(801, (dim,)) + 1.0, rnd(802, (dim,))
    lp = Layout(rows, dim)

    def run(x_, with_y=True):
        y = oc.sentinel_buffer(lp, F32)
        hi, lo = oc.sentinel_buffer(lp, F16), oc.sentinel_buffer(lp, F16)
        slot = torch.zeros(8, device="cuda")
        check(lib().loco_op_layernorm_f16x3(ptr(x_), ptr(g), ptr(b), oc.base(y, lp) if with_y else None, oc.base(hi, lp), oc.base(lo, lp), ptr(slot),
                                            rows, dim, 1e-5, stream()))
        torch.cuda.synchronize()
        oc.assert_guards(hi, lp, "layernorm hi")
        oc.assert_guards(lo, lp, "layernorm lo")
        return y, hi, lo, slot

    y, hi, lo, slot = run(x)
    oc.assert_guards(y, lp, "layernorm y")
    yo = oc.owned(y, lp).view(rows, dim)
    want_hi = yo.half()
    assert oc.same_bits(oc.owned(hi, lp).view(rows, dim), want_hi), "hi != fp16(y)"
    assert oc.same_bits(oc.owned(lo, lp).view(rows, dim), (yo - want_hi.float()).half()), "lo != fp16(y - hi)"
    ref = F.layer_norm(x.double().cpu(), (dim,), g.double().cpu(), b.double().cpu(), 1e-5)
    rl2 = float((yo.double().cpu() - ref).norm() / ref.norm())
    assert rl2 < 2e-6, rl2
    assert not bool(slot.any())
    _, hi2, lo2, _ = run(x, with_y=False)  # the forward's own call: planes only
    assert oc.same_bits(hi2, hi) and oc.same_bits(lo2, lo)
    bad = x.clone()
    r_bad = rows // 2
    bad[r_bad, dim // 3] = float("nan")
    _, hi3, lo3, slot3 = run(bad)
    assert float(slot3.max()) == float("inf") and int((slot3 != 0).sum()) == 1
    keep = torch.arange(rows, device="cuda") != r_bad
    for got, clean in ((hi3, hi), (lo3, lo)):
        assert oc.same_bits(oc.owned(got, lp).view(rows, dim)[keep].contiguous(), oc.owned(clean, lp).view(rows, dim)[keep].contiguous())
