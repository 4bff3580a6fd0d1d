"""-m gpu: the waveform front end pinned per element -- frame counts, the normaliser, conv0 + GroupNorm + GELU in both output forms
(loco_op_conv0_gn_gelu_ex), the fp32 positional conv, and guard bands round the small LayerNorm launches.

Inputs, fp64 references and bars: tests/frontend_cases.py and tests/op_check.py (tests/test_frontend_ref.py checks on the CPU that the
bars hold a float32 restatement and catch each named defect).  Every output lives in a sentinel-filled allocation that must come back
untouched outside what the operator owns; inputs are followed by NaN.  Where the source promises identical bits they are compared:
mask forms, a row alone and inside its batch, in place, a second launch, the planes and the fp16 split of the fp32 form, t0_clip and the
clip alone.  Paths these cases enter that no other operator test does:
  mask_count_kernel        rows off a 16-byte boundary (the scalar loop), the one-element tail behind the int4 loop, two parts
  frames_from_counts       n < 10 (floor division of a negative n - k), every n in 0 .. 1200
  wav_moments / apply      n < 128 (empty parts), n = 0 and 1, L > 524288 (the grid-stride loop's second trip)
  conv0_moments_kernel     T0 < 64 (empty parts), T0 = 16385 (a thread's second trip)
  conv0_apply_kernel<true> planes, the range word, t0_clip's zeros
  pos_conv_kernel          the halo, tile edges and the position gather per element; single taps at a bar of a few u
"""
import ctypes as C
import functools

import pytest
import torch

import frontend_cases as fc
import value_domain_cases as vd

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import op_check as oc
    from gpu_util import check, lib, ptr, stream
    from op_check import Layout, knobs

F16, F32 = torch.float16, torch.float32
SENT32 = 0x7FC0BEEF


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def bits_of(value):
    return int(torch.tensor([value], dtype=F32).view(torch.int32))


def assert_outside_untouched(buf, layout, what):
    """the guard half of oc.assert_guards, for a region (scratch) the operator need not fill"""
    mask = torch.ones(layout.total, dtype=torch.bool, device="cuda")
    mask[layout.index().reshape(-1)] = False
    touched = torch.nonzero(mask & (bits(buf) != oc.SENTINEL[buf.dtype])).reshape(-1)
    assert touched.numel() == 0, f"{what}: {touched.numel()} guard elements overwritten, first at flat offset {int(touched[0]) - layout.head}"


def poisoned2d(x):
    """x [rows, cols] (CPU or device) inside NaN: (buffer, layout)"""
    l = Layout(x.shape[0], x.shape[1])
    return oc.poisoned(x.cuda().reshape(1, 1, *x.shape), l), l


# ---- frame counts -----------------------------------------------------------------------------------------------------------------
def run_frames(mask, B, L):
    buf = torch.full((64 + B + 256,), SENT32, dtype=torch.int32, device="cuda")
    if mask is not None:
        assert mask.data_ptr() % 16 == 0 and mask.is_contiguous()
    check(lib().loco_op_frame_counts(ptr(mask), B, L, C.c_void_p(buf.data_ptr() + 256), stream()))
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENT32).all()) and bool((buf[64 + B:] == SENT32).all()), "frame counts: a word outside frames[0 .. B) was written"
    return buf[64:64 + B].cpu().tolist()


def test_frame_counts_every_length_to_1200():
    want = [fc.frames_ref(n) for n in range(fc.SWEEP_L + 1)]
    assert run_frames(fc.sweep_mask().cuda(), fc.SWEEP_L + 1, fc.SWEEP_L) == want
    assert [lib().loco_output_frames(n) for n in range(fc.SWEEP_L + 1)] == want
    assert min(want) < 0 < max(want)


def test_frame_counts_unaligned_rows_tail_and_holes():
    prefix, holes = fc.unaligned_masks()
    want = [fc.frames_ref(n) for n in fc.UNALIGNED_LENGTHS]
    assert run_frames(prefix.cuda(), 5, fc.UNALIGNED_L) == want
    assert run_frames(holes.cuda(), 5, fc.UNALIGNED_L) == want
    assert run_frames(None, 5, fc.UNALIGNED_L) == [fc.frames_ref(fc.UNALIGNED_L)] * 5
    assert run_frames(None, 3, 7) == [fc.frames_ref(7)] * 3


# ---- normaliser -------------------------------------------------------------------------------------------------------------------
def run_norm(x, mask, pad=fc.NORM_PAD, in_place=False):
    """loco_op_normalize_waveform on x [B, L] (CPU) -> out [B, L] (device); output and scratch guarded, scratch exactly what is asked"""
    B, L = x.shape
    lo = Layout(B, L)
    nbytes = int(lib().loco_normalize_scratch_bytes(B))
    ls = Layout(1, nbytes // 4)
    scratch = oc.sentinel_buffer(ls, F32)
    md = mask.cuda() if mask is not None else None
    if in_place:
        out = oc.sentinel_buffer(lo, F32)
        out[lo.index().reshape(-1)] = x.cuda().reshape(-1)
        src = oc.base(out, lo)
    else:
        xin, li = poisoned2d(x)
        out = oc.sentinel_buffer(lo, F32)
        src = oc.base(xin, li)
    check(lib().loco_op_normalize_waveform(src, ptr(md), B, L, pad, oc.base(out, lo), oc.base(scratch, ls), nbytes, stream()))
    torch.cuda.synchronize()
    oc.assert_guards(out, lo, "normaliser output")
    assert_outside_untouched(scratch, ls, "normaliser scratch")
    return oc.owned(out, lo).view(B, L)


def check_norm(name, out, x, counts, **tags):
    ref, bar, S = fc.norm_reference(x, counts)
    live = torch.arange(x.shape[1])[None] < torch.tensor(counts)[:, None]
    o = out.cpu()
    assert bool((bits(o)[~live] == bits_of(fc.NORM_PAD)).all()), f"{name}: an element at i >= n does not hold the padding value's bits"
    sel = live & (bar > 0)
    assert bool((o[live & ~sel] == 0).all())
    oc.assert_elements(name, o[sel], ref[sel], S[sel], bar[sel], **tags)


def test_normaliser_ragged_counts():
    x, mask = fc.norm_ragged()
    out = run_norm(x, mask)
    check_norm("normalize", out, x, fc.NORM_COUNTS, case="ragged")
    assert bool((bits(out[0]) == bits_of(fc.NORM_PAD)).all()), "n = 0: not all padding"
    assert int(bits(out[1, :1])) == 0, "n = 1: the one sample is not +0.0"
    # a row alone is the row inside its batch; in place is out of place; a second launch is the first
    for b in range(x.shape[0]):
        assert oc.same_bits(run_norm(x[b:b + 1], mask[b:b + 1]), out[b:b + 1].contiguous()), f"row {b} alone differs from row {b} in the batch"
    assert oc.same_bits(run_norm(x, mask, in_place=True), out), "in place differs from out of place"
    assert oc.same_bits(run_norm(x, mask), out), "second launch differs"


def test_normaliser_mask_forms():
    x = fc.norm_full()
    out = run_norm(x, None)
    check_norm("normalize", out, x, [fc.NORM_L] * x.shape[0], case="no mask")
    assert oc.same_bits(run_norm(x, torch.ones(x.shape, dtype=torch.int32)), out), "a mask of ones differs from no mask"
    assert oc.same_bits(run_norm(x, None, in_place=True), out), "in place differs from out of place"


def test_normaliser_grid_stride_second_trip():
    x, mask = fc.norm_long()
    out = run_norm(x, mask)
    check_norm("normalize", out, x, [int(mask.sum())], case="L = 524588")
    assert oc.same_bits(run_norm(x, mask, in_place=True), out), "in place differs from out of place"


# ---- conv0 + GroupNorm + GELU -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv0_dev():
    return tuple(t.cuda() for t in fc.conv0_weights())


@functools.lru_cache(maxsize=None)
def conv0_ref(name):
    x, _ = fc.conv0_input(name)
    return fc.conv0_reference(x, fc.CONV0_CLIP if name == "clip" else None)


def run_conv0(x, form, t0_clip=None, slot=None):
    """form "f32" / "planes": loco_op_conv0_gn_gelu_ex, "old": loco_op_conv0_gn_gelu.  -> fp32 [B, T0, 512] or (hi, lo)"""
    B, L = x.shape
    T0 = (L - 10) // 5 + 1
    xin, li = poisoned2d(x)
    lo = Layout(B * T0, 512)
    w, gw, gb = conv0_dev()
    scratch = torch.empty(int(lib().loco_conv0_scratch_bytes(B)), dtype=torch.uint8, device="cuda")
    tc = torch.tensor(t0_clip, dtype=torch.int32, device="cuda") if t0_clip is not None else None
    outs = [oc.sentinel_buffer(lo, F32)] if form != "planes" else [oc.sentinel_buffer(lo, F16), oc.sentinel_buffer(lo, F16)]
    if form == "old":
        check(lib().loco_op_conv0_gn_gelu(oc.base(xin, li), B, L, ptr(w), ptr(gw), ptr(gb), oc.base(outs[0], lo), ptr(scratch), stream()))
    else:
        o = [oc.base(outs[0], lo), None, None] if form == "f32" else [None, oc.base(outs[0], lo), oc.base(outs[1], lo)]
        check(lib().loco_op_conv0_gn_gelu_ex(oc.base(xin, li), B, L, ptr(w), ptr(gw), ptr(gb), *o, slot, ptr(tc), ptr(scratch), stream()))
    torch.cuda.synchronize()
    for o in outs:
        oc.assert_guards(o, lo, f"conv0 {form}")
    outs = [oc.owned(o, lo).view(B, T0, 512) for o in outs]
    return outs[0] if form != "planes" else tuple(outs)


def check_conv0(name, case, x, t0_clip=None):
    """both forms of one input against the bar; planes == the split of the fp32 form; the old op and a second launch the same bits"""
    out = run_conv0(x, "f32", t0_clip)
    hi, lo = run_conv0(x, "planes", t0_clip)
    ref, bar, S = conv0_ref(case)
    live = bar > 0
    oc.assert_elements(name, out.cpu()[live], ref[live], S[live], bar[live], case=case, form="f32")
    assert bool((bits(out.cpu())[~live] == 0).all()), f"{case}: a frame at or beyond t0_clip is not +0.0"
    want_hi, want_lo = vd.expected_split(out.cpu())
    assert oc.same_bits(hi.cpu(), want_hi), f"{case}: hi plane is not fp16(out)"
    assert oc.same_bits(lo.cpu(), want_lo), f"{case}: lo plane is not fp16(out - hi)"
    bar_p = oc.planes_bar(bar, ref)
    oc.assert_elements(name, (hi.double() + lo.double()).cpu()[live], ref[live], S[live], bar_p[live], case=case, form="planes")
    assert oc.same_bits(run_conv0(x, "f32", t0_clip), out), f"{case}: second launch differs"
    hi2, lo2 = run_conv0(x, "planes", t0_clip)
    assert oc.same_bits(hi2, hi) and oc.same_bits(lo2, lo), f"{case}: second plane launch differs"
    if t0_clip is None:
        assert oc.same_bits(run_conv0(x, "old"), out), f"{case}: loco_op_conv0_gn_gelu differs from _ex with out"
    return out, hi, lo


@pytest.mark.parametrize("T0", fc.CONV0_SMALL_T0)
def test_conv0_small_t0(T0):
    x, _ = fc.conv0_input(f"small{T0}")
    assert x.shape == (3, fc.conv0_len(T0, fc.CONV0_SMALL_T0.index(T0)))
    check_conv0("conv0", f"small{T0}", x)


def test_conv0_moments_second_trip():
    x, _ = fc.conv0_input("large")
    assert (x.shape[1] - 10) // 5 + 1 == fc.CONV0_LARGE_T0
    check_conv0("conv0", "large", x)


@pytest.mark.parametrize("case", fc.CONV0_HOSTILE)
def test_conv0_hostile_clips(case):
    x, _ = fc.conv0_input(case)
    out, hi, lo = check_conv0("conv0", case, x)
    if case == "silence":
        assert oc.same_bits(out, out[:, :1].expand_as(out).contiguous()), "silence: a column is not one value"


def test_conv0_rejects_both_and_neither_output():
    x = torch.zeros(1, 64, device="cuda")
    w, gw, gb = conv0_dev()
    scratch = torch.empty(int(lib().loco_conv0_scratch_bytes(1)), dtype=torch.uint8, device="cuda")
    o32, o16 = torch.empty(11 * 512, device="cuda"), torch.empty(11 * 512, dtype=F16, device="cuda")
    for o in ((None, None, None), (ptr(o32), ptr(o16), ptr(o16)), (None, ptr(o16), None), (ptr(o32), None, ptr(o16))):
        assert lib().loco_op_conv0_gn_gelu_ex(ptr(x), 1, 64, ptr(w), ptr(gw), ptr(gb), *o, None, None, ptr(scratch), stream()) != 0


def test_conv0_range_word():
    x, _ = fc.conv0_input("small129")
    out = run_conv0(x, "f32")
    ls = Layout(1, 8)
    slot = oc.sentinel_buffer(ls, F32)
    slot[ls.head:ls.head + 8] = 0.0
    run_conv0(x, "planes", slot=oc.base(slot, ls))
    oc.assert_guards(slot, ls, "range words")
    words = bits(oc.owned(slot, ls).reshape(8))
    top = int(bits(out.abs().max().reshape(1)))
    assert int(words.max()) == top, f"range words' maximum {int(words.max()):#x} is not max |out| = {top:#x}"
    # T0 = 129: blocks 0, 1, 2 of each clip feed words 0, 1, 2; the others stay zero
    per_shard = [int(bits(out[:, 64 * i:64 * (i + 1)].abs().max().reshape(1))) for i in range(3)]
    assert words.tolist() == per_shard + [0] * 5, f"range words {words.tolist()} are not the blocks' maxima {per_shard}"
    slot[ls.head:ls.head + 8] = 1e30
    run_conv0(x, "planes", slot=oc.base(slot, ls))
    oc.assert_guards(slot, ls, "range words")
    assert bool((bits(oc.owned(slot, ls).reshape(8)) == bits_of(1e30)).all()), "a range word above every value was changed"


def test_conv0_t0_clip_is_the_clip_alone():
    x, _ = fc.conv0_input("clip")
    out, hi, lo = check_conv0("conv0", "clip", x, fc.CONV0_CLIP)
    for b, tc in enumerate(fc.CONV0_CLIP):
        alone = x[b:b + 1, :fc.conv0_len(tc)].contiguous()
        assert oc.same_bits(run_conv0(alone, "f32"), out[b:b + 1, :tc].contiguous()), f"clip {b}: frames below t0_clip differ from the clip alone"
        ahi, alo = run_conv0(alone, "planes")
        assert oc.same_bits(ahi, hi[b:b + 1, :tc].contiguous()) and oc.same_bits(alo, lo[b:b + 1, :tc].contiguous())
        assert not bool(bits(out[b, tc:]).any()) and not bool(bits(hi[b, tc:]).any()) and not bool(bits(lo[b, tc:]).any())


# ---- positional conv, fp32 --------------------------------------------------------------------------------------------------------
def run_pos(h, wf, bias, tab, frames):
    B, T, _ = h.shape
    hin, lh = poisoned2d(h.reshape(B * T, 768))
    tin, lt = poisoned2d(tab)
    lo = Layout(B * T, 768)
    out = oc.sentinel_buffer(lo, F32)
    fr = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    check(lib().loco_op_pos_conv(oc.base(hin, lh), ptr(wf), ptr(bias), oc.base(tin, lt), ptr(fr), oc.base(out, lo), B, T, stream()))
    torch.cuda.synchronize()
    oc.assert_guards(out, lo, "pos_conv output")
    return oc.owned(out, lo).view(B, T, 768)


@functools.lru_cache(maxsize=None)
def pos_dev():
    w, bias = fc.pos_weights32()
    return fc.fold(w).cuda(), bias.cuda()


@pytest.mark.parametrize("B,T,frames", fc.POS_SHAPES)
def test_pos_conv_per_element(B, T, frames):
    h, tab = fc.pos_input(B, T)
    w, bias = fc.pos_weights32()
    ref, bar, S = fc.pos_reference(h, w, bias, tab, frames)
    wf, bd = pos_dev()
    out = run_pos(h, wf, bd, tab, frames)
    oc.assert_elements("posconv_f32", out, ref, S, bar, rel_l2_bar=2e-6, B=B, T=T)
    assert oc.same_bits(run_pos(h, wf, bd, tab, frames), out), "second launch differs"


@functools.lru_cache(maxsize=None)
def shift_ref(T, tap, value, fp16_exact):
    h, tab = fc.pos_input(1, T, fp16_exact)
    _, bias = fc.pos_weights32()
    return fc.pos_reference(h, fc.one_hot_weight(tap, value), bias, tab, None, count=1)


@pytest.mark.parametrize("T", fc.SHIFT_T)
def test_pos_conv_single_taps(T):
    """one-hot weights: out = h + GELU(h[t + tap - 64] + bias) + table to the GELU rule and two additions"""
    h, tab = fc.pos_input(1, T)
    _, bd = pos_dev()
    for tap in fc.SHIFT_TAPS:
        ref, bar, S = shift_ref(T, tap, 1.0, False)
        out = run_pos(h, fc.fold(fc.one_hot_weight(tap)).cuda(), bd, tab, None)
        oc.assert_elements("posconv_f32_shift", out, ref, S, bar, T=T, tap=tap)


def run_pos_f16x3(h, whi, wlo, bias, out_scale, tab, ws=None):
    B, T, _ = h.shape
    hd = h.cuda().contiguous()
    lg = Layout(B * 16 * (T + 128), 48, tail=oc.TILE_SLACK * 49 + 15 * 16 * (T + 128) * 48)
    lo = Layout(B * T, 768, tail=oc.TILE_SLACK * 769 + 15 * T * 768)
    ghi, glo, out = oc.sentinel_buffer(lg, F16), oc.sentinel_buffer(lg, F16), oc.sentinel_buffer(lo, F32)
    td = tab.cuda()
    check(lib().loco_op_pos_conv_f16x3(ptr(hd), ptr(whi), ptr(wlo), ptr(bias), ptr(td), None, None, out_scale, 3, oc.base(ghi, lg), oc.base(glo, lg),
                                       ptr(ws), ws.numel() * 4 if ws is not None else 0, oc.base(out, lo), B, T, stream()))
    torch.cuda.synchronize()
    for b_, l_ in ((ghi, lg), (glo, lg), (out, lo)):
        oc.assert_guards(b_, l_, "positional conv f16x3")
    return oc.owned(out, lo).view(B, T, 768)


@pytest.mark.parametrize("T", fc.SHIFT_T)
def test_pos_conv_f16x3_single_taps(T):
    """the same single taps through loco_op_pos_conv_f16x3 in every form: h is fp16-exact (lo = 0), the weight plane holds one power of two
    per output channel and out_scale is the product path's own (pos_weights() of test_gpu_gemm_contract.py): the product is exact"""
    from test_gpu_gemm_contract import pos_weights, splitk_ws
    _, _, out_scale, bias, _ = pos_weights()
    plane = 2.0 ** 13
    assert bool((bias.cpu() == fc.pos_weights32()[1]).all())
    h, tab = fc.pos_input(1, T, True)
    for tap in fc.SHIFT_TAPS:
        ref, bar, S = shift_ref(T, tap, plane * out_scale, True)
        wg = fc.one_hot_weight(tap, plane).view(16, 48, 48, 128).permute(0, 1, 3, 2).reshape(16, 48, 6144).contiguous()
        whi, wlo = wg.half().cuda(), torch.zeros(16, 48, 6144, dtype=F16, device="cuda")
        for path, env, ws in (("automatic", {}, None), ("NI=2", dict(LOCO_POSCONV_NI="2"), None), ("NI=4", dict(LOCO_POSCONV_NI="4"), None),
                              ("generic", dict(LOCO_POSCONV_GENERIC="1"), None), ("split-K", {}, splitk_ws())):
            with knobs(**env):
                out = run_pos_f16x3(h, whi, wlo, bias, out_scale, tab, ws)
            oc.assert_elements("posconv_f16x3_shift", out, ref, S, bar, T=T, tap=tap, path=path)


# ---- LayerNorm, small launches inside guards --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [512, 768])
@pytest.mark.parametrize("rows", [1, 5])
def test_layernorm_small_launches_stay_inside(rows, dim):
    import torch.nn.functional as F
    x = fc.hu(f"fe.ln.x.{rows}.{dim}", (rows, dim), 3.0).cuda() + 0.5
    r = fc.hu(f"fe.ln.r.{rows}.{dim}", (rows, dim), 1.0).cuda()
    g, b = fc.hu("fe.ln.g", (dim,)).cuda() + 1.0, fc.hu("fe.ln.b", (dim,)).cuda()
    rhi, rlo = oc.split_planes(r)
    lp = Layout(rows, dim)
    xin, lx = poisoned2d(x)

    def fresh():
        return oc.sentinel_buffer(lp, F32), oc.sentinel_buffer(lp, F16), oc.sentinel_buffer(lp, F16)

    def verify(y, hi, lo, x64, what):
        for buf in (y, hi, lo):
            if buf is not None:
                oc.assert_guards(buf, lp, what)
        ref = F.layer_norm(x64, (dim,), g.double().cpu(), b.double().cpu(), 1e-5)
        if y is not None:
            yo = oc.owned(y, lp).view(rows, dim)
            assert float((yo.double().cpu() - ref).norm() / ref.norm()) < 2e-6, what
            if hi is not None:
                want_hi, want_lo = vd.expected_split(yo.cpu())
                assert oc.same_bits(oc.owned(hi, lp).view(rows, dim).cpu(), want_hi) and oc.same_bits(oc.owned(lo, lp).view(rows, dim).cpu(), want_lo), what
        else:
            got = oc.owned(hi, lp).double().cpu() + oc.owned(lo, lp).double().cpu()
            assert float((got.view(rows, dim) - ref).norm() / ref.norm()) < 2e-6, what

    y, _, _ = fresh()
    check(lib().loco_op_layernorm(oc.base(xin, lx), ptr(g), ptr(b), oc.base(y, lp), rows, dim, 1e-5, stream()))
    torch.cuda.synchronize()
    verify(y, None, None, x.double().cpu(), "loco_op_layernorm")
    y, hi, lo = fresh()
    check(lib().loco_op_layernorm_f16x3(oc.base(xin, lx), ptr(g), ptr(b), oc.base(y, lp), oc.base(hi, lp), oc.base(lo, lp), None, rows, dim, 1e-5, stream()))
    torch.cuda.synchronize()
    verify(y, hi, lo, x.double().cpu(), "loco_op_layernorm_f16x3")
    y, hi, lo = fresh()
    check(lib().loco_op_layernorm_f16x3_residual(oc.base(xin, lx), ptr(rhi), ptr(rlo), ptr(g), ptr(b), oc.base(y, lp), oc.base(hi, lp), oc.base(lo, lp),
                                                 None, rows, dim, 1e-5, stream()))
    torch.cuda.synchronize()
    verify(y, hi, lo, x.double().cpu() + rhi.double().cpu() + rlo.double().cpu(), "loco_op_layernorm_f16x3_residual")
    _, hi, lo = fresh()
    check(lib().loco_op_layernorm_f16x3_residual(oc.base(xin, lx), ptr(rhi), ptr(rlo), ptr(g), ptr(b), None, oc.base(hi, lp), oc.base(lo, lp),
                                                 None, rows, dim, 1e-5, stream()))
    torch.cuda.synchronize()
    verify(None, hi, lo, x.double().cpu() + rhi.double().cpu() + rlo.double().cpu(), "loco_op_layernorm_f16x3_residual, planes only")
