"""The residual of the encoder's out-projection and second FFN GEMM is added by the LayerNorm behind them (norm_misc.hip, RESID).

Op level: loco_op_layernorm_f16x3_residual(x, rhi, rlo) must give the BITS of loco_op_layernorm_f16x3 on the host-side float32 sum
x + (float32(rhi) + float32(rlo)) -- the same two IEEE additions in the same order, nothing that could contract -- in both planes and
in y, and leave 64 sentinel elements before and after every output untouched.
Forward level: a ragged pair through two layers against the oracle at the parity bar of tests/test_gpu_encoder.py, and its full-length
clip alone (B = 1: other split-K slices than inside the pair) against its rows of the pair.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import op_check as oc
    from gpu_util import check, la, lib, model, ptr, rel_l2, stream
    from op_check import Layout

F16, F32 = torch.float16, torch.float32
TOL = 2e-5  # tests/test_gpu_encoder.py
GUARD = 64


def ln_case(rows, dim):
    """x with one row of large values and one all-zero row (from 3 rows on; fewer rows cannot hold both beside an ordinary one),
    the residual as planes of a random fp32 tensor, and the float32 sum formed on the host."""
    rng = np.random.default_rng(900 + 7 * rows + dim)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    if rows >= 3:
        x[rows // 2] = (1e4 * rng.standard_normal(dim)).astype(np.float32)
        x[0] = 0.0
    r = (2.0 * rng.standard_normal((rows, dim))).astype(np.float32)
    hi = r.astype(np.float16)
    lo = (r - hi.astype(np.float32)).astype(np.float16)
    total = x + (hi.astype(np.float32) + lo.astype(np.float32))
    assert total.dtype == np.float32
    g = (rng.random(dim) + 0.5).astype(np.float32)
    b = rng.standard_normal(dim).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()
    return dev(x), dev(hi), dev(lo), dev(total), dev(g), dev(b)


@pytest.mark.parametrize("dim", [512, 768])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 65])
def test_residual_layernorm_has_the_bits_of_layernorm_on_the_sum(rows, dim):
    x, rhi, rlo, total, g, b = ln_case(rows, dim)
    lp = Layout(rows, dim, head=GUARD, tail=GUARD)

    def run(resid, with_y):
        y = oc.sentinel_buffer(lp, F32)
        hi, lo = oc.sentinel_buffer(lp, F16), oc.sentinel_buffer(lp, F16)
        slot = torch.zeros(8, device="cuda")
        out = (oc.base(y, lp) if with_y else None, oc.base(hi, lp), oc.base(lo, lp), ptr(slot), rows, dim, 1e-5, stream())
        if resid:
            check(lib().loco_op_layernorm_f16x3_residual(ptr(x), ptr(rhi), ptr(rlo), ptr(g), ptr(b), *out))
        else:
            check(lib().loco_op_layernorm_f16x3(ptr(total), ptr(g), ptr(b), *out))
        torch.cuda.synchronize()
        oc.assert_guards(hi, lp, "hi")
        oc.assert_guards(lo, lp, "lo")
        if with_y:
            oc.assert_guards(y, lp, "y")
        else:
            assert oc.same_bits(y, oc.sentinel_buffer(lp, F32)), "y written although not requested"
        assert not bool(slot.any())
        return y, hi, lo

    for with_y in (True, False):
        want, got = run(False, with_y), run(True, with_y)
        for name, w, o in zip(("y", "hi", "lo"), want, got):
            assert oc.same_bits(o, w), f"{name} (y requested: {with_y}) differs from LayerNorm of the host-side sum"
    assert bool(torch.isfinite(oc.owned(got[1], lp).float()).all())


def test_residual_planes_go_together():
    x, rhi, rlo, _, g, b = ln_case(4, 768)
    hi, lo = torch.empty(4, 768, dtype=F16, device="cuda"), torch.empty(4, 768, dtype=F16, device="cuda")
    for a_hi, a_lo in ((ptr(rhi), None), (None, ptr(rlo))):
        rc = lib().loco_op_layernorm_f16x3_residual(ptr(x), a_hi, a_lo, ptr(g), ptr(b), None, ptr(hi), ptr(lo), None, 4, 768, 1e-5, stream())
        assert rc == -1, rc  # LOCO_E_INVALID
        assert b"loco_op_layernorm_f16x3_residual" in lib().loco_last_error()


def test_ragged_pair_against_the_oracle_and_its_long_clip_alone(oracle):
    """5 s + 3 s, two layers: the parity bar of the encoder tests.  The 5 s clip alone (M = 249 against 498: the split-K GEMMs cut K
    into other slices, and their reduction kernel now stores without the residual) is deterministic, meets the same bar, and agrees
    with its rows inside the pair as far as tests/test_gpu_encoder.py asks of two schedules with different K slices (5e-6; that file
    asks bit equality only of clips that run the same slices, and neither do these)."""
    m, sd = model(layers=2)
    enc = m.speecht5.encoder
    x, msk = la.synth.batch([80000, 48000])
    y = enc(input_values=torch.from_numpy(x).cuda(), attention_mask=torch.from_numpy(msk).cuda()).last_hidden_state
    assert tuple(y.shape) == (2, 249, 768)
    assert rel_l2(y, oracle.encode(x, msk, sd)) < TOL
    x1, m1 = la.synth.batch([80000])
    assert np.array_equal(x1[0], x[0])
    one = enc(input_values=torch.from_numpy(x1).cuda(), attention_mask=torch.from_numpy(m1).cuda()).last_hidden_state
    again = enc(input_values=torch.from_numpy(x1).cuda(), attention_mask=torch.from_numpy(m1).cuda()).last_hidden_state
    assert torch.equal(one, again)
    assert rel_l2(one, oracle.encode(x1, m1, sd)) < TOL
    assert rel_l2(one[0], y[0]) < 5e-6
