"""CPU self-test of tests/value_domain_cases.py: the references and bars the GPU tests of the value domain lean on are themselves held
to figures here, so that a GPU test can only fail for what the kernel did.

1. the GELU polynomial restated in fp32 (exact exp2) meets the figures the bars are built from, and the bars are those figures plus the
   documented 1 ulp of v_exp_f32          2. expected_split reconstructs x to the 22 bits the format gives, and the ties are ties
3. the softmax / LayerNorm builders do what their names say, and torch's CPU fp32 evaluation of them stays well inside the project's
   fixed bars: the reference alone never uses up a bar
"""
import numpy as np
import pytest
import torch

import intent_head_oracle as iho
import value_domain_cases as vd

F32 = np.float32


# ---- 1. GELU ------------------------------------------------------------------------------------------------------------------------------
def test_gelu_grid_holds_what_it_names():
    grid, specials = vd.gelu_grid()
    assert grid.dtype == F32 and bool(np.isfinite(grid).all()) and grid.size == 4096 + 90 + 2 + 3 + 6 + 6
    assert grid.min() == F32(-1e30) and grid.max() == F32(1e30)
    for v in (vd.K_SMAX, -vd.K_SMAX, np.nextafter(vd.K_SMAX, F32(9)), np.nextafter(-vd.K_SMAX, F32(-9)), F32(2.0 ** -149), F32(-2.0 ** -149), F32(2.0 ** -40),
              F32(-16.0), np.finfo(F32).tiny):
        assert (grid == v).any(), v
    assert bool(np.signbit(grid[grid == 0]).any()) and not bool(np.signbit(grid[grid == 0]).all())
    assert np.isposinf(specials[0]) and np.isneginf(specials[1]) and np.isnan(specials[2])
    sub = vd.gelu_subgrid(249)
    assert sub.size == 249 and set(sub.tolist()) <= set(grid.tolist())
    assert (sub == vd.K_SMAX).any() and (sub == -vd.K_SMAX).any() and (sub == F32(-2.0 ** -149)).any() and (sub < vd.TAIL).sum() > 30


def test_gelu_ref64_is_the_erf_form_where_that_one_is_accurate():
    x = np.linspace(-3.0, 9.0, 1001)
    want = 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x) / np.sqrt(2.0)).numpy())
    assert np.abs(vd.gelu_ref64(x) - want).max() <= 1e-15 * 9
    # the negative tail against the asymptotic series of erfc: x phi(x) / |x| (1 - 1/x^2 + 3/x^4 - 15/x^6 + 105/x^8)
    t = np.asarray([-8.0, -9.0])
    series = -np.exp(-t * t / 2) / np.sqrt(2 * np.pi) * (1 - 1 / t ** 2 + 3 / t ** 4 - 15 / t ** 6 + 105 / t ** 8)
    assert np.abs(vd.gelu_ref64(t) / series - 1).max() < 2e-4
    sp = vd.gelu_ref64(np.asarray([np.inf, -np.inf, np.nan, 0.0, -0.0]))
    assert np.isposinf(sp[0]) and sp[1] == 0 and np.isnan(sp[2]) and sp[3] == 0 and sp[4] == 0


def test_restated_gelu_meets_the_figures_the_bars_are_built_from():
    grid, specials = vd.gelu_grid()
    fig = vd.gelu_errors(grid, vd.gelu_restated32(grid))
    print("gelu_restated32 against float64:", fig)
    assert fig["pos_rel"][0] <= vd.RESTATED_POS_REL, fig
    assert fig["neg_rel"][0] <= vd.RESTATED_NEG_REL, fig
    assert fig["tail_abs"][0] <= vd.RESTATED_TAIL_ABS, fig
    assert fig["neg_abs_per_x"][0] <= vd.RESTATED_NEG_ABS_PER_X, fig
    # ... and they are figures of THIS polynomial, not slack: each is reached to within three tenths
    assert fig["pos_rel"][0] >= 0.7 * vd.RESTATED_POS_REL and fig["neg_rel"][0] >= 0.7 * vd.RESTATED_NEG_REL
    assert fig["tail_abs"][0] >= 0.7 * vd.RESTATED_TAIL_ABS and fig["neg_abs_per_x"][0] >= 0.7 * vd.RESTATED_NEG_ABS_PER_X
    # the bars: the figure plus one ulp of h = erfc / 2 <= 1/2 -- 2^-23 of (1 - h) >= 1/2, 2^-23 of x h
    assert vd.RESTATED_POS_REL + 2.0 ** -23 <= vd.BAR_POS_REL <= 1.05 * (vd.RESTATED_POS_REL + 2.0 ** -23)
    assert vd.RESTATED_NEG_REL + 2.0 ** -23 <= vd.BAR_NEG_REL <= 1.2 * (vd.RESTATED_NEG_REL + 2.0 ** -23)
    assert vd.RESTATED_TAIL_ABS * (1 + 2.0 ** -23) <= vd.BAR_TAIL_ABS <= 1.3 * vd.RESTATED_TAIL_ABS
    sp = vd.gelu_restated32(specials)
    assert np.isposinf(sp[0]) and abs(float(sp[1])) <= vd.BAR_TAIL_ABS and np.isnan(sp[2])
    z = vd.gelu_restated32(np.asarray([0.0, -0.0], F32))
    assert z[0] == 0 and z[1] == 0


def test_a_seventh_digit_of_the_last_coefficient_shows():
    """What the GPU test must be able to see: 1.151104808 -> 1.151105808 moves -5.7 <= x < 0 past its bar."""
    grid, _ = vd.gelu_grid()
    fig = vd.gelu_errors(grid, vd.gelu_restated32(grid, last_coefficient=1.151105808))
    assert fig["neg_rel"][0] > vd.BAR_NEG_REL, fig


# ---- 2. the plane split -------------------------------------------------------------------------------------------------------------------
def test_split_values_hold_every_fp16_number_and_every_tie():
    v = vd.split_values()
    assert v.shape == (256, 1024) and v.dtype == F32
    flat = v.reshape(-1)
    have = set(flat[np.isfinite(flat)].view(np.uint32).tolist())
    h = np.arange(1, 0x7C00, dtype=np.uint16).view(np.float16).astype(F32)
    mid = vd.split_ties()
    assert mid.size == 0x7BFF and mid[0] == F32(2.0 ** -25) and mid[-1] == F32(65488.0)
    for part in (h, -h, mid, -mid, np.nextafter(mid, F32(0)), np.nextafter(-mid, F32(-1e9))):
        assert set(part.view(np.uint32).tolist()) <= have
    for s in (65504.0, 65519.996, 65520.0, 1e5, 2.0 ** -149, 2.0 ** -15, 2.0 ** -40, -65520.0):
        assert F32(s).view(np.uint32) in have, s
    assert np.isnan(flat).sum() == 2 and np.isinf(flat).sum() == 2
    # a tie is a tie: fp16(mid) is the neighbour with the even significand, and the two fp32 neighbours go to the two sides
    t = torch.from_numpy(mid)
    bits = t.half().view(torch.int16).int()
    assert bool((bits % 2 == 0).all())
    lo_side = torch.from_numpy(np.nextafter(mid, F32(0))).half().view(torch.int16).int()
    hi_side = torch.from_numpy(np.nextafter(mid, F32(1e9))).half().view(torch.int16).int()
    assert bool((hi_side - lo_side == 1).all()) and bool(((bits == lo_side) | (bits == hi_side)).all())
    nar = vd.split_narrow_values(253, 12)
    assert nar.shape == (253, 12) and np.isnan(nar).sum() == 2 and (nar == F32(65520.0)).any()
    assert len(set(nar.reshape(-1).view(np.uint32).tolist()) & set(mid.view(np.uint32).tolist())) > 200


def test_expected_split_reconstructs_22_bits():
    x = torch.from_numpy(vd.split_values()).reshape(-1)
    hi, lo = vd.expected_split(x)
    ok = torch.isfinite(x) & (x.abs() < 65504)
    rec = hi.double() + lo.double()
    err = (rec - x.double()).abs()[ok].numpy()
    assert bool((err <= vd.split_bound(x[ok].numpy())).all())
    assert bool(vd.hi_is_nearest(hi[ok], lo[ok]).all())
    same = rec[ok].float().half() == hi[ok]
    assert 0 < int((~same).sum()) <= 2 * 0x7C00   # half(hi + lo) != hi happens, at fp32 neighbours of ties only
    assert bool((lo[ok].double().abs().numpy() <= vd.ulp_f16(hi[ok].double().numpy()) / 2).all())
    # the edge: 65504 and everything below the tie stay finite, the tie 65520 and beyond round to inf with lo = -inf
    edge = torch.tensor([65504.0, float(np.nextafter(F32(65520.0), F32(0))), 65520.0, 1e5, float("inf"), float("nan"), -0.0])
    h, l_ = vd.expected_split(edge)
    assert h[:2].tolist() == [65504.0, 65504.0] and l_[0] == 0 and float(l_[1]) == 16.0
    assert bool(torch.isposinf(h[2:5]).all()) and bool(torch.isneginf(l_[2:4]).all()) and bool(torch.isnan(l_[4])) and bool(torch.isnan(h[5]))
    assert vd.ulp_f16(np.asarray([1.0, 1.5, 2.0, 2.0 ** -14, 2.0 ** -20, 0.0])).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]


# ---- 3. the builders ------------------------------------------------------------------------------------------------------------------------
BAR_ATTN, BAR_PROBS = 1e-5, 1e-5   # tests/test_gpu_decoder.py, tests/test_gpu_decoder_attn.py
BAR_HEAD, BAR_HEAD_DQ = 2e-5, 1e-5  # tests/test_gpu_intent_head.py


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def scores(q, k):
    B, Sq, Tk = q.shape[0], q.shape[1], k.shape[1]
    return vd.SCALE * torch.einsum("bihd,bjhd->bhij", q.double().view(B, Sq, 12, 64), k.double().view(B, Tk, 12, 64))


@pytest.mark.parametrize("Tk", [600, 200])
@pytest.mark.parametrize("kind", vd.ATTN_KINDS)
def test_decoder_attention_cases(kind, Tk):
    Sq = 3
    q, k, v = vd.decoder_attention_case(kind, Sq, Tk)
    s = scores(q, k)
    if kind.startswith("lead"):
        j = min(int(kind[4:]), Tk - 1)
        others = torch.cat([s[..., :j], s[..., j + 1:]], -1).amax(-1)
        assert float((s[..., j] - others).min()) >= vd.LEAD - 1e-3 and float((s[..., j] - others).max()) < vd.LEAD + 25
    elif kind == "ascending":
        assert float(s.diff(dim=-1).min()) > 0 and float((s[..., 64:] - s[..., :-64]).min()) > 0.9 * vd.ASCENT
    else:
        assert bool((k == k[:, :1]).all()) and float((s - s[..., :1]).abs().max()) == 0.0
    for causal, offset in ((0, 0), (1, Tk - Sq)):
        ref = vd.attention_ref(q, k, v, None, causal, offset)
        own = vd.attention_ref(q, k, v, None, causal, offset, torch.float32)
        assert rel_l2(own, ref) <= BAR_ATTN / 4
        assert float((vd.row_bar(ref, own) / ref.abs().clamp(min=1.0)).max()) <= BAR_ATTN


@pytest.mark.parametrize("Tk", [65, 257])
@pytest.mark.parametrize("kind", vd.PROBS_KINDS)
def test_decoder_probs_cases(kind, Tk):
    """The two launches of the GPU test: key counts on B = 2, Sq = 3, and the causal square B = 1, Sq = Tk."""
    assert (Tk - 1) // 64 == (Tk + 63) // 64 - 1 >= 1   # the last key sits in the row's last tile, and that is not the first
    for B, Sq, counts, causal in ((2, 3, [Tk, Tk - 3], False), (2, 3, None, False), (1, Tk, None, True)):
        q, k = vd.decoder_probs_case(kind, B, Sq, Tk)
        s = scores(q, k)
        if kind == "last":
            assert float((s[..., -1] - s[..., :-1].amax(-1)).min()) >= vd.LEAD - 1e-3
        else:
            assert float(s.diff(dim=-1).min()) > 0 and float((s[..., 64:] - s[..., :-64]).min()) > 0.9 * vd.ASCENT
        ref, _ = vd.probs_ref(q, k, counts, causal)
        own, _ = vd.probs_ref(q, k, counts, causal, torch.float32)
        assert float((own.double() - ref).abs().max()) <= BAR_PROBS / 4
        assert float(vd.row_bar(ref, own).max()) <= BAR_PROBS
        assert float((own.double().sum(-1) - 1).abs().max()) <= BAR_PROBS / 4


@pytest.mark.parametrize("T", [300, 129])
def test_head_batches(T):
    q = vd.head_query()
    W, b = vd.head_params()
    x, target = vd.head_batch(T, q)
    z = x.double() @ q.double()
    assert float(z[0].diff().min()) > 0 and abs(float(z[0, -1]) - 24.0) < 1e-3
    for a in range(128, T, 128):
        assert float(z[0, a:a + 128].max() - z[0, a - 128:a].max()) > 0.05   # every split raises the maximum
    lead1 = z[1, T - 1] - z[1, :T - 1].max()
    lead2 = z[2, T // 3] - torch.cat([z[2, :T // 3], z[2, T // 3 + 1:]]).max()
    assert abs(float(lead1) - 30.0) < 1e-3 and abs(float(lead2) - 80.0) < 1e-3
    assert (T - 1) // 128 == (T + 127) // 128 - 1 >= 1   # frame T - 1 sits in the last split, and that is not the first
    alpha32 = torch.softmax((x @ q), -1)
    assert float(alpha32[2, T // 3]) == 1.0 and float(alpha32[2].sort().values[-2]) < 2.0 ** -110   # the other weights vanish from an fp32 sum
    ref = vd.head_reference(iho.IntentClassifierOracle, q, W, b, x, target, torch.float64)
    own = vd.head_reference(iho.IntentClassifierOracle, q, W, b, x, target, torch.float32)
    fig = {k_: rel_l2(own[k_], ref[k_]) for k_ in ref}
    print("torch fp32 head against float64, T =", T, fig)
    for k_ in ("logits", "loss", "dW", "db"):
        assert fig[k_] <= BAR_HEAD / 4, fig
    assert fig["dq"] <= BAR_HEAD_DQ / 4, fig


@pytest.mark.parametrize("dim", [768, 512])
def test_layernorm_rows(dim):
    x, g, b = vd.layernorm_rows(dim)
    assert x.shape == (5, dim)
    assert abs(float(x[0].mean()) - 1e3) < 0.2 and 0.8 < float(x[0].double().std()) < 1.2
    assert float(x[1].max()) == 1e4 and float(x[1].abs().sort().values[-2]) < 6
    assert float(x[2].double().var()) < 1e-5 / 100
    ref, own = vd.layernorm_ref(x, g, b, torch.float64), vd.layernorm_ref(x, g, b, torch.float32)
    print("torch fp32 LayerNorm against float64, per row:", (own.double() - ref).abs().amax(-1).tolist())
    assert rel_l2(own[1:], ref[1:]) <= 2e-6   # tests/test_gpu_ops.py test_layernorm's bar; the row around 1e3 loses the bits of its mean
    assert 2e-6 < float((own[0].double() - ref[0]).abs().max()) < 1e-3
