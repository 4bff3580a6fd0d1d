"""The bars of the front end's per-element contract (tests/op_check.py: normalize_bar, conv0_bar, pos_conv_bar) are neither vacuous nor
too tight, checked without a GPU: for every case of tests/frontend_cases.py a plain float32 restatement of the operator stays within
the bar of the fp64 reference, and a restatement with one named defect leaves it (or the integer equality) on at least one element.
A defect that stays inside means the case is too weak: the case is fixed, never the bar.
"""
import pytest
import torch

import frontend_cases as fc


def assert_within(name, out, ref, bar):
    at = fc.first_over(out, ref, bar)
    assert at is None, f"{name}: restatement leaves its bar at element {at}: {float(out[at])} vs {float(ref[at])}, bar {float(bar[at]):.3e}"
    live = bar > 0
    print(f"{name}: max err / bar = {float(((out.double() - ref).abs()[live] / bar[live]).max()) if bool(live.any()) else 0.0:.4f}")


def assert_caught(name, sabotage, out, ref, bar):
    at = fc.first_over(out, ref, bar)
    assert at is not None, f"{name}: sabotage '{sabotage}' stays inside the bar on every element"
    print(f"{name}: sabotage '{sabotage}' caught, first at element {at}: {float(out[at])} vs {float(ref[at])}, bar {float(bar[at]):.3e}")


# ---- frame counts -----------------------------------------------------------------------------------------------------------------
def test_frame_chain_is_the_library_s_python_one_and_truncation_is_caught(synth):
    ns = list(range(fc.SWEEP_L + 1)) + fc.UNALIGNED_LENGTHS + [480000, 9600000]
    assert [fc.frames_ref(n) for n in ns] == [synth.conv_out_length(n) for n in ns]
    assert fc.frames_ref(400) == 1 and fc.frames_ref(399) == 0 and fc.frames_ref(480000) == 1499
    assert fc.sweep_mask().sum(1).tolist() == list(range(fc.SWEEP_L + 1))
    prefix, holes = fc.unaligned_masks()
    assert prefix.sum(1).tolist() == holes.sum(1).tolist() and not torch.equal(prefix, holes)
    wrong = [n for n in range(fc.SWEEP_L + 1) if fc.frames_ref(n, "truncate") != fc.frames_ref(n)]
    assert wrong and min(wrong) < 10, "truncating division is not caught for n < 10"
    print(f"frame chain: sabotage 'truncate' caught at n = {wrong[:12]} ... ({len(wrong)} of {fc.SWEEP_L + 1})")


# ---- normaliser -------------------------------------------------------------------------------------------------------------------
def test_normaliser_restated_and_sabotaged():
    x, _ = fc.norm_ragged()
    ref, bar, _ = fc.norm_reference(x, fc.NORM_COUNTS)
    out = fc.norm_restated(x, fc.NORM_COUNTS)
    assert_within("normaliser ragged", out, ref, bar)
    assert float(out[1, 0]) == 0.0 and bool((out[0] == fc.NORM_PAD).all())
    for sabotage in ("n+1", "unbiased"):
        assert_caught("normaliser ragged", sabotage, fc.norm_restated(x, fc.NORM_COUNTS, sabotage=sabotage), ref, bar)
    # n + 1 is caught by more than the NaN behind n: also where the sample behind the row's end is an ordinary one
    xf = fc.norm_full()
    counts = [fc.NORM_L - 1] * xf.shape[0]
    ref, bar, _ = fc.norm_reference(xf, counts)
    assert_within("normaliser full", fc.norm_restated(xf, counts), ref, bar)
    assert_caught("normaliser full", "n+1", fc.norm_restated(xf, counts, sabotage="n+1"), ref, bar)
    assert_caught("normaliser full", "unbiased", fc.norm_restated(xf, counts, sabotage="unbiased"), ref, bar)


def test_normaliser_long_row_restated():
    x, mask = fc.norm_long()
    n = int(mask.sum())
    ref, bar, _ = fc.norm_reference(x, [n])
    assert_within("normaliser long", fc.norm_restated(x, [n]), ref, bar)


# ---- conv0 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"small{t}" for t in fc.CONV0_SMALL_T0] + ["large"] + fc.CONV0_HOSTILE)
def test_conv0_restated(name):
    x, _ = fc.conv0_input(name)
    ref, bar, _ = fc.conv0_reference(x)
    out = fc.conv0_restated(x)
    assert bool(torch.isfinite(out).all())
    assert_within(f"conv0 {name}", out, ref, bar)
    if name == "silence":
        assert bool((out == out[:, :1]).all()), "silence: a column is not one value"


def test_conv0_sabotaged():
    for name, sabotage in (("small129", "unpadded"), ("small129", "T0-1"), ("small129", "window+1"), ("small65", "T0-1"),
                           ("small64", "window+1"), ("large", "T0-1")):
        x, lengths = fc.conv0_input(name)
        ref, bar, _ = fc.conv0_reference(x)
        assert_caught(f"conv0 {name}", sabotage, fc.conv0_restated(x, lengths, sabotage), ref, bar)


def test_conv0_t0_clip_reference_is_the_clip_alone():
    """the reference with t0_clip: rows below it are the clip alone at the length whose T0 is t0_clip[b], rows beyond are zero with a zero bar"""
    x, _ = fc.conv0_input("clip")
    ref, bar, _ = fc.conv0_reference(x, fc.CONV0_CLIP)
    for b, tc in enumerate(fc.CONV0_CLIP):
        alone, _, _ = fc.conv0_reference(x[b:b + 1, :fc.conv0_len(tc)].contiguous())
        assert torch.equal(ref[b, :tc], alone[0])
        assert not bool(ref[b, tc:].any()) and not bool(bar[b, tc:].any()) and bool((bar[b, :tc] > 0).all())


# ---- positional conv --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,frames", fc.POS_SHAPES)
def test_pos_conv_restated_and_sabotaged(B, T, frames):
    h, tab = fc.pos_input(B, T)
    w, bias = fc.pos_weights32()
    ref, bar, _ = fc.pos_reference(h, w, bias, tab, frames)
    assert_within(f"pos_conv {B}x{T}", fc.pos_restated(h, w, bias, tab, frames), ref, bar)
    assert tab.unique(dim=0).shape[0] == T + 2
    for sabotage in ("pos+1", "pad_last") + (("tap+1", "group") if T > 1 else ()) + (("no_drop",) if B > 1 else ()):
        assert_caught(f"pos_conv {B}x{T}", sabotage, fc.pos_restated(h, w, bias, tab, frames, sabotage), ref, bar)


@pytest.mark.parametrize("T", fc.SHIFT_T)
def test_pos_conv_shift_cases_restated_and_sabotaged(T):
    """one-hot weights: the conv is the single exact product h[t + tap - 64]; the bar is a few u and sees a tap or a group off by one"""
    h, tab = fc.pos_input(1, T)
    _, bias = fc.pos_weights32()
    for tap in fc.SHIFT_TAPS:
        w = fc.one_hot_weight(tap)
        ref, bar, _ = fc.pos_reference(h, w, bias, tab, None, count=1)
        shifted = torch.zeros_like(h)
        lo, hi = max(0, 64 - tap), min(T, T + 64 - tap)
        shifted[:, lo:hi] = h[:, lo + tap - 64:hi + tap - 64]
        want = h.double() + fc.oc.gelu64(shifted.double() + bias.double()) + tab.double()[fc.positions(1, T, None)]
        assert float((ref - want).abs().max()) < 1e-12, "the one-hot reference is not the shift"
        assert float((bar / (fc.oc.U * (h.double().abs() + tab.double()[fc.positions(1, T, None)].abs() + 1))).max()) < 12, "the shift bar is not a few u"
        assert_within(f"pos_conv shift T={T} tap={tap}", fc.pos_restated(h, w, bias, tab, None), ref, bar)
        for sabotage in ("tap+1", "group"):
            assert_caught(f"pos_conv shift T={T} tap={tap}", sabotage, fc.pos_restated(h, w, bias, tab, None, sabotage), ref, bar)
