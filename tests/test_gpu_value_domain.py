"""-m gpu: GELU, the fp16 plane split and LayerNorm on the values where they can be wrong (inputs and references: value_domain_cases.py).

GELU, element by element.  Every kernel that compiles gelu_erf / gelu_erf2 is launched with ZERO A and W (zero planes for the
split-precision GEMM): the accumulator is +0, the pre-activation is bias[n] exactly, every row of the output must be bit-identical to
row 0, and row 0 is compared per element with 0.5 x erfc(-x / sqrt 2) in float64.  Bars (value_domain_cases.py; the polynomial's own
CPU figure, asserted by test_value_domain_ref.py, plus the documented 1 ulp of v_exp_f32):
    x > 0  3e-7 relative     -5.7 <= x < 0  4e-6 relative     x < -5.7 and -inf  2.5e-8 absolute     +-0 -> 0     +inf -> +inf     NaN -> NaN
Two things follow from the number formats and are added to a bar, never to what the polynomial may do: one subnormal quantum
2^-149 (a result below FLT_MIN has no relative accuracy), and, where the output is read back as fp16 hi + lo planes, the planes' own
max(2^-22 |y|, 2^-25) (value_domain_cases.split_bound; at |y| >= 65520 hi must be +inf instead).
conv0's GELU cannot be given exact pre-activations through its operator (they come out of its GroupNorm): it stays with
test_gpu_ops.test_conv0_groupnorm_gelu.

The plane split, bit for bit: loco_op_split_f16 (plain C++) and split_f16_2pairs (the inline-asm v_fma_mix* form of the GEMM epilogues,
reached with zero planes and the values as the residual R) on every fp16 number, every tie, the ties' fp32 neighbours, the 65504 / 65520
edge, the subnormals of lo -- through every tile form, the split-K reduction and the narrow store path n + 16 > N (N = 1036).

LayerNorm on rows far from N(0, 1), per row against float64 with torch's CPU fp32 F.layer_norm as the yardstick (the rule of
tests/test_gpu_decoder_score.py).
"""
import contextlib
import math
import os

import numpy as np
import pytest
import torch

import value_domain_cases as vd
from conftest import record_figure

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpu_util import check, dev, la, lib, ptr, stream

F32 = np.float32
TILES = [0, 1, 2, 3, 4, 5, 6, 7, 8]  # 0: the dispatch's own choice


@contextlib.contextmanager
def tile_form(tile):
    """LOCO_GEMM_TILE for the launches inside, as test_gemm_f16x3_every_tile_form_agrees_bit_for_bit sets it."""
    try:
        if tile:
            os.environ["LOCO_GEMM_TILE"] = str(tile)
            lib().loco_debug_reload_gemm_knobs()
        yield
    finally:
        os.environ.pop("LOCO_GEMM_TILE", None)
        lib().loco_debug_reload_gemm_knobs()


_zeros = {}


def zeros(shape, dtype=torch.float32):
    key = (tuple(shape), dtype)
    if key not in _zeros:
        _zeros[key] = torch.zeros(shape, dtype=dtype, device="cuda")
    return _zeros[key]


def gelu_columns(width):
    """The grid and the specials as rows of `width` pre-activations, the last row padded with 1.0."""
    grid, specials = vd.gelu_grid()
    x = np.concatenate([specials, grid])
    rows = -(-x.size // width)
    out = np.ones(rows * width, F32)
    out[:x.size] = x
    return out.reshape(rows, width)


def check_gelu(name, x, got, split=False, **where):
    """x fp32 pre-activations, got float64 (fp32 output, or hi + lo) with `hi` given for the split kind: assert the bars, record the worst."""
    hi = where.pop("hi", None)
    x = np.asarray(x, F32).reshape(-1)
    got = np.asarray(got, np.float64).reshape(-1)
    ref = vd.gelu_ref64(x)
    big = np.abs(ref) >= 65520.0 if split else np.zeros(x.shape, bool)   # fp16(y) is inf from here on
    fin = np.isfinite(x) & ~big
    fig = vd.gelu_errors(x[fin], got[fin])
    fmt = vd.split_bound(ref) if split else np.zeros(x.shape)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
    rel_bar = vd.SUBNORMAL_QUANTUM + fmt
    bad = []
    for sel, bar in ((fin & (x > 0), vd.BAR_POS_REL * np.abs(ref) + rel_bar), (fin & (x < 0) & (x >= vd.TAIL), vd.BAR_NEG_REL * np.abs(ref) + rel_bar),
                     ((fin & (x < vd.TAIL)) | np.isneginf(x), vd.BAR_TAIL_ABS + fmt)):
        miss = sel & ~(err <= bar)
        bad += [(float(a), float(b), float(c)) for a, b, c in zip(x[miss][:5], got[miss][:5], ref[miss][:5])]
    zero = x == 0
    assert zero.any() and bool((got[zero] == 0).all()), (name, where, got[zero])
    top = hi.reshape(-1) if split else got
    assert np.isposinf(x).any() and bool(np.isposinf(top[np.isposinf(x) | (big & (ref > 0))]).all()), (name, where)
    assert np.isnan(x).any() and bool(np.isnan(top[np.isnan(x)]).all()) and bool(np.isnan(got[np.isnan(x)]).all()), (name, where)
    assert bool(np.isfinite(got[fin]).all()), (name, where)
    record_figure("gelu_value_domain", kernel=name, split_output=split, **where, **{k: v[0] for k, v in fig.items()}, **{k + "_at": v[1] for k, v in fig.items()})
    print("GELU", name, "split" if split else "fp32", where, {k: f"{v[0]:.3g} at {v[1]:.6g}" for k, v in fig.items()})
    assert not bad, (name, where, "x, got, float64:", bad)
    return fig


def rows_equal_row0(t):
    """Every row bit-identical to row 0 (int views: NaNs compare by their bits)."""
    v = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return bool((v == v[:1]).all())


def run_f16x3(bias, M, N, K, out_split, epi=1, R=None, A=None, W=None, splitk=False):
    """loco_op_gemm_f16x3 / _splitk; A, W = (hi, lo) planes or None for zero planes.  Returns C, or (Chi, Clo)."""
    ahi, alo = A if A is not None else (zeros((M, K), torch.float16),) * 2
    whi, wlo = W if W is not None else (zeros((N, K), torch.float16),) * 2
    C_ = torch.full((M, N), -7.0, device="cuda")
    ldp = (N + 7) // 8 * 8  # planes leave as 16-byte pieces: their row stride is a multiple of 8 halves (N = 1036: 1040)
    chi = torch.full((M, ldp), -7.0, dtype=torch.float16, device="cuda")
    clo = torch.full((M, ldp), -7.0, dtype=torch.float16, device="cuda")
    out = (None, ptr(chi), ptr(clo)) if out_split else (ptr(C_), None, None)
    ldc = ldp if out_split else N
    if splitk:
        ws = torch.empty(int(lib().loco_gemm_splitk_bytes()), dtype=torch.uint8, device="cuda")
        check(lib().loco_op_gemm_f16x3_splitk(ptr(ahi), ptr(alo), K, ptr(whi), ptr(wlo), K, ptr(bias), ptr(R), N, *out, ldc, M, N, K, epi, ptr(ws), ws.numel(),
                                              stream()), "gemm_f16x3_splitk")
    else:
        check(lib().loco_op_gemm_f16x3(ptr(ahi), ptr(alo), K, ptr(whi), ptr(wlo), K, ptr(bias), ptr(R), N, *out, ldc, M, N, K, epi, 1, 1, 0, 0, 0, 0, stream()),
              "gemm_f16x3")
    torch.cuda.synchronize()
    return (chi[:, :N].contiguous(), clo[:, :N].contiguous()) if out_split else C_


def gelu_through_f16x3(name, cols, out_split, splitk=False, also=None, **where):
    """GELU(cols[l, n]) through the split-precision GEMM, one launch per row of cols; `also`: a column slice checked and recorded by itself."""
    M, N, K = 130, cols.shape[1], 512 if splitk else 32
    got, his = [], []
    for row in cols:
        out = run_f16x3(dev(row), M, N, K, out_split, splitk=splitk)
        if out_split:
            assert rows_equal_row0(out[0]) and rows_equal_row0(out[1]), (name, where)
            got.append((out[0][0].double() + out[1][0].double()).cpu().numpy())
            his.append(out[0][0].double().cpu().numpy())
        else:
            assert rows_equal_row0(out), (name, where)
            got.append(out[0].double().cpu().numpy())
    got, his = np.stack(got), np.stack(his) if out_split else None
    if also is not None:
        check_gelu(name, cols[:, also], got[:, also], split=out_split, hi=his[:, also] if out_split else None, columns=f"{also.start}:", **where)
    return check_gelu(name, cols, got, split=out_split, hi=his, **where)


# ---- B. GELU ------------------------------------------------------------------------------------------------------------------------------
def test_gelu_fp32_gemm():
    cols = gelu_columns(1024)
    M, N, K = 130, 1024, 32
    A, W = zeros((M, K)), zeros((N, K))
    got = []
    for row in cols:
        C_ = torch.full((M, N), -7.0, device="cuda")
        b = dev(row)
        check(lib().loco_op_gemm(ptr(A), K, ptr(W), K, ptr(b), None, N, ptr(C_), N, M, N, K, 1, 1, 1, 0, 0, 0, 0, stream()), "gemm")
        torch.cuda.synchronize()
        assert rows_equal_row0(C_)
        got.append(C_[0].double().cpu().numpy())
    check_gelu("gemm_f32", cols, np.stack(got))


@pytest.mark.parametrize("tile", TILES)
def test_gelu_gemm_f16x3_every_tile_form(tile):
    cols = gelu_columns(1024)   # N = 1024 = 4 x 256: every form may be forced
    with tile_form(tile):
        for out_split in (False, True):
            gelu_through_f16x3("gemm_f16x3", cols, out_split, tile=tile)


def test_gelu_gemm_f16x3_splitk_reduction():
    cols = gelu_columns(1024)
    for out_split in (False, True):
        gelu_through_f16x3("splitk_reduce", cols, out_split, splitk=True, K=512)   # M = 130, K = 512: two slices of 256


def test_gelu_gemm_f16x3_narrow_store_path():
    """N = 1036: the last 16-column run of a row holds 12 columns, n + 16 > N, and split_gemm_store16 falls back to the 4-column store.  The
    specials and a 249-point subgrid go through those 12 columns, 12 per launch; the other 1024 columns carry the grid as before."""
    _, specials = vd.gelu_grid()
    last = np.concatenate([specials, vd.gelu_subgrid(249)]).reshape(21, 12)
    wide = gelu_columns(1024)
    cols = np.concatenate([wide[np.arange(21) % len(wide)], last], axis=1)
    assert cols.shape == (21, 1036)
    for out_split in (False, True):
        gelu_through_f16x3("gemm_f16x3", cols, out_split, also=slice(1024, 1036), N=1036)


def test_gelu_skinny_gemm():
    cols = gelu_columns(1024)
    M, N, K = 5, 1024, 256
    A, W = zeros((M, K)), zeros((N, K))
    got = []
    for row in cols:
        C_ = torch.full((M, N), -7.0, device="cuda")
        b = dev(row)
        check(lib().loco_op_skinny_gemm(ptr(A), K, ptr(W), K, ptr(b), None, N, ptr(C_), N, M, N, K, 1, stream()), "skinny_gemm")
        torch.cuda.synchronize()
        assert rows_equal_row0(C_)
        got.append(C_[0].double().cpu().numpy())
    check_gelu("skinny_gemm", cols, np.stack(got))


def test_gelu_pos_conv():
    """h = 0, weights = 0, a zero sinusoid table: out[t, c] = 0 + GELU(0 + bias[c]) + 0, 768 values per launch."""
    cols = gelu_columns(768)
    B, T = 1, 70
    h, wf, tab = zeros((B, T, 768)), zeros((16, 128, 48, 48)), zeros((T + 2, 768))
    got = []
    for row in cols:
        out = torch.full((B, T, 768), -7.0, device="cuda")
        b = dev(row)
        check(lib().loco_op_pos_conv(ptr(h), ptr(wf), ptr(b), ptr(tab), None, ptr(out), B, T, stream()), "pos_conv")
        torch.cuda.synchronize()
        assert rows_equal_row0(out[0])
        got.append(out[0, 0].double().cpu().numpy())
    check_gelu("pos_conv", cols, np.stack(got))


# ---- C. the plane split, bit for bit ------------------------------------------------------------------------------------------------------
def assert_planes_equal(got_hi, got_lo, x, what):
    """int16 views equal to expected_split(x); a NaN is compared by its position."""
    want_hi, want_lo = vd.expected_split(x)
    for name, got, want in (("hi", got_hi.cpu(), want_hi), ("lo", got_lo.cpu(), want_lo)):
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), (what, name, "NaN positions differ")
        diff = (got.view(torch.int16) != want.view(torch.int16)) & ~nan
        n = int(diff.sum())
        if n:
            i = diff.reshape(-1).nonzero()[:6, 0]
            raise AssertionError((what, name, n, "x, got, want:", list(zip(torch.as_tensor(x).reshape(-1)[i].tolist(), got.reshape(-1)[i].tolist(),
                                                                            want.reshape(-1)[i].tolist()))))


def test_split_op_on_every_fp16_number_tie_and_edge():
    x = torch.from_numpy(vd.split_values())
    xd = dev(x)
    hi = torch.full(x.shape, -7.0, dtype=torch.float16, device="cuda")
    lo = torch.full(x.shape, -7.0, dtype=torch.float16, device="cuda")
    check(lib().loco_op_split_f16(ptr(xd), ptr(hi), ptr(lo), xd.numel(), stream()))
    torch.cuda.synchronize()
    assert_planes_equal(hi, lo, x, "loco_op_split_f16")


@pytest.mark.parametrize("mode", ["natural", "tile1", "tile2", "tile3", "tile4", "tile5", "tile6", "tile7", "tile8", "splitk", "narrow"])
def test_split_in_the_gemm_epilogue_bit_for_bit(mode):
    """Zero planes, epilogue 2: the kernel writes the planes of 0.0f + R (a -0 becomes +0) through split_f16_2pairs."""
    v = torch.from_numpy(vd.split_values())
    if mode == "narrow":   # N = 1036: hostile values of their own in the last 12 columns (the 4-column store path)
        v = torch.cat([v[:253], torch.from_numpy(vd.split_narrow_values(253, 12))], dim=1)
    M, N = v.shape
    R = dev(v)
    with tile_form(int(mode[4:]) if mode.startswith("tile") else 0):
        chi, clo = run_f16x3(None, M, N, 512 if mode == "splitk" else 32, True, epi=2, R=R, splitk=mode == "splitk")
    assert_planes_equal(chi, clo, torch.zeros(()) + v, mode)


_real = {}


def real_operands():
    if not _real:
        M, N, K = 130, 1024, 96
        hu = lambda key, shape, scale: torch.from_numpy(la.synth.hashed_uniform(key, shape, 11)) * scale  # noqa: E731
        A, W, b = hu("vd.a", (M, K), 2.0), hu("vd.w", (N, K), 2.0 / math.sqrt(K)), hu("vd.b", (N,), 1.0)
        _real.update(A=vd.expected_split(A), W=vd.expected_split(W), b=b)
    return tuple(t.cuda() for t in _real["A"]), tuple(t.cuda() for t in _real["W"]), dev(_real["b"])


@pytest.mark.parametrize("tile", TILES)
def test_split_planes_of_real_gelu_outputs(tile):
    """Hashed operands, epilogue 1: the planes against the fp32 output of the same arguments.  hi is a nearest fp16 number of hi + lo
    (half(hi + lo) == hi, but for a sum that is exactly a tie: value_domain_cases.hi_is_nearest), |lo| <= ulp(hi) / 2, and hi + lo is the
    fp32 value to max(2^-22 |C|, 2^-25) -- bounds of the format, not measurements."""
    A, W, b = real_operands()
    M, N, K = 130, 1024, 96
    with tile_form(tile):
        C_ = run_f16x3(b, M, N, K, False, A=A, W=W).cpu()
        chi, clo = (t.cpu() for t in run_f16x3(b, M, N, K, True, A=A, W=W))
    assert bool(torch.isfinite(C_).all()) and float(C_.abs().max()) > 1.0
    rec = chi.double() + clo.double()
    # the issue's half(hi + lo) == hi, but for a sum that is EXACTLY a tie (the fp32 value one step beside a tie has its lo rounded to half
    # a spacing): there hi and half(hi + lo) are the two fp16 numbers equally near the sum -- asserted, not assumed
    rounded = rec.float().half()
    differs = rounded.view(torch.int16) != chi.view(torch.int16)
    assert bool(((rec - chi.double()).abs() == (rec - rounded.double()).abs())[differs].all())
    assert bool(vd.hi_is_nearest(chi, clo).all())
    exact_ties = int(differs.sum())
    assert bool((clo.double().abs().numpy() <= vd.ulp_f16(chi.double().numpy()) / 2).all())
    ratio = float(((rec - C_.double()).abs().numpy() / vd.split_bound(C_.numpy())).max())
    record_figure("split_planes_real_data", tile=tile, worst_over_format_bound=ratio, sums_that_are_exact_ties=exact_ties)
    assert ratio <= 1.0, ratio


# ---- E. LayerNorm on hostile rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [768, 512])
def test_layernorm_hostile_rows(dim):
    x, g, b = vd.layernorm_rows(dim)
    ref, own = vd.layernorm_ref(x, g, b, torch.float64), vd.layernorm_ref(x, g, b, torch.float32)
    bar = vd.row_bar(ref, own)
    xd, gd, bd, y = dev(x), dev(g), dev(b), torch.full((5, dim), -7.0, device="cuda")
    check(lib().loco_op_layernorm(ptr(xd), ptr(gd), ptr(bd), ptr(y), 5, dim, 1e-5, stream()))
    torch.cuda.synchronize()
    err = (y.double().cpu() - ref).abs()
    fig = dict(err=err.amax(-1).tolist(), torch_fp32=(own.double() - ref).abs().amax(-1).tolist(), over_bar=(err / bar).amax(-1).tolist())
    record_figure("layernorm_hostile_rows", dim=dim, **fig)
    print("LayerNorm hostile rows", dim, fig)
    assert bool(torch.isfinite(y).all()) and bool((err <= bar).all()), fig
    check(lib().loco_op_layernorm(ptr(xd), ptr(gd), ptr(bd), ptr(xd), 5, dim, 1e-5, stream()))  # in place
    torch.cuda.synchronize()
    assert torch.equal(xd, y)
