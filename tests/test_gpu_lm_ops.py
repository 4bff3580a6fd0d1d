"""-m gpu: the language model's three new device pieces as operators -- the fused LM head (loco_op_lm_head_nll), the gelu_new GEMM
epilogue (loco_op_gemm, epilogue 5) and the embedding (loco_op_lm_embed) -- against float64.

Bars.  The head multiplies fp32 numbers and sums 768 products per logit, then 50 257 exponentials: so does a plain fp32 evaluation of the
same formula on the CPU (torch: h @ w.T, logsumexp, minus the target's logit), whose own distance from float64 is measured here on the
same inputs.  The bar is 4 x the larger of that figure and one ulp of the largest NLL of the case (2^-23 |nll|): the same class of error,
in another order, and a result cannot be asked to be better than its own rounding."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import lm_ref
import value_domain_cases as vd
from conftest import record_figure
from gpu_util import check, dev, lib, ptr, stream

pytestmark = pytest.mark.gpu
IGNORE = -100
F32 = np.float32


def head(h, w, t, V=None):
    R, V = h.shape[0], V or w.shape[0]
    nb = int(lib().loco_lm_head_scratch_bytes(R, V))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    out = torch.full((R,), -7.0, device="cuda")
    check(lib().loco_op_lm_head_nll(ptr(h), 768, ptr(w), 768, ptr(t), R, V, IGNORE, ptr(out), ptr(scratch), nb, stream()), "lm_head_nll")
    torch.cuda.synchronize()
    return out


_cases = {}


def case(V):
    """130 rows and V weight rows, their float64 NLLs and the fp32 CPU evaluation's error: computed once per V, shared by every R."""
    if V not in _cases:
        rng = np.random.default_rng(1000 + V)
        h = rng.standard_normal((130, 768)).astype(F32)
        w = (rng.standard_normal((V, 768)) * 0.1).astype(F32)           # logits of standard deviation 2.8
        t = rng.integers(0, V, 130).astype(np.int32)
        ref = lm_ref.head_nll(h, w, t)
        z32 = torch.from_numpy(h) @ torch.from_numpy(w).T
        cpu32 = (torch.logsumexp(z32, -1) - z32[torch.arange(130), torch.from_numpy(t).long()]).double().numpy()
        _cases[V] = dict(h=h, w=w, t=t, ref=ref, cpu_err=np.abs(cpu32 - ref), dw=dev(w))
    return _cases[V]


def bar_of(cpu_err, ref):
    return 4.0 * max(float(np.max(cpu_err)), 2.0 ** -23 * float(np.nanmax(np.abs(ref))))


@pytest.mark.parametrize("V", [64, 1003, 50257])
@pytest.mark.parametrize("R", [1, 33, 130])
def test_head_against_float64(R, V):
    c = case(V)
    got = head(dev(c["h"][:R]), c["dw"], dev(c["t"][:R], torch.int32)).double().cpu().numpy()
    err = float(np.abs(got - c["ref"][:R]).max())
    bar = bar_of(c["cpu_err"][:R], c["ref"][:R])
    record_figure("lm_head_nll", R=R, V=V, max_abs_err=err, cpu_fp32_err=float(c["cpu_err"][:R].max()), bar=bar, mean_nll=float(c["ref"][:R].mean()))
    print("lm_head_nll", R, V, "err", err, "cpu fp32", float(c["cpu_err"][:R].max()), "bar", bar)
    assert err <= bar


def test_head_row_is_independent_of_the_launch():
    """The same row and target scored alone, as row 0 of 33 and as row 129 of 130: the same bits."""
    c = case(50257)
    row, tgt = c["h"][7], c["t"][7]
    outs = []
    for R, at in ((1, 0), (33, 0), (130, 129)):
        h, t = c["h"][:R].copy(), c["t"][:R].copy()
        h[at], t[at] = row, tgt
        outs.append(head(dev(h), c["dw"], dev(t, torch.int32))[at].view(torch.int32).item())
    assert outs[0] == outs[1] == outs[2], outs
    assert abs(np.int32(outs[0]).view(F32) - c["ref"][7]) <= bar_of(c["cpu_err"][7:8], c["ref"][7:8])


def test_head_hostile_rows():
    V = 1003
    c = case(V)
    w = c["w"].copy()
    w[500] = w[20]                                         # two equal rows: two bit-identical logits
    unit = lambda j: w[j].astype(np.float64) / float((w[j].astype(np.float64) ** 2).sum())  # noqa: E731
    rows, tg = [], []
    rows.append((80.0 * unit(7)).astype(F32)); tg.append(7)        # logit 7 = +80, the maximum, and the target
    rows.append((-80.0 * unit(7)).astype(F32)); tg.append(7)       # logit 7 = -80, the minimum, and the target
    rows.append((80.0 * unit(7)).astype(F32)); tg.append(900)      # +80 elsewhere, the target in another chunk's tile
    rows.append((30.0 * unit(20)).astype(F32)); tg.append(500)     # two equal maxima (20 and 500), one of them the target
    nan_row = c["h"][0].copy(); nan_row[5] = np.nan
    inf_row = c["h"][1].copy(); inf_row[3] = np.inf
    rows += [nan_row, inf_row, c["h"][2], c["h"][3], c["h"][4], nan_row]
    tg += [3, 3, V, -1, IGNORE, IGNORE]                            # ... an out-of-range, a negative and two ignored targets
    h = np.stack(rows)
    t = np.asarray(tg, np.int32)
    got = head(dev(h), dev(w), dev(t, torch.int32)).double().cpu().numpy()
    ref = lm_ref.head_nll(h, w, t)
    z = h[:4].astype(np.float64) @ w.astype(np.float64).T
    assert abs(z[0, 7] - 80) < 1e-3 and z[0].argmax() == 7 and abs(z[1, 7] + 80) < 1e-3 and z[1].argmin() == 7 and z[3, 20] == z[3, 500] == z[3].max()
    assert np.isnan(got[4]) and np.isnan(got[5]) and np.isnan(got[6]) and np.isnan(got[7]) and got[8] == 0.0 and got[9] == 0.0, got
    z32 = torch.from_numpy(h[:4]) @ torch.from_numpy(w).T
    cpu32 = (torch.logsumexp(z32, -1) - z32[torch.arange(4), torch.from_numpy(t[:4]).long()]).double().numpy()
    bar = bar_of(np.abs(cpu32 - ref[:4]), ref[:4])
    err = np.abs(got[:4] - ref[:4])
    record_figure("lm_head_nll_hostile", err=err.tolist(), ref=ref[:4].tolist(), bar=bar)
    print("hostile", got[:4], ref[:4], "bar", bar)
    assert (err <= bar).all() and got[0] >= 0.0 and abs(got[3] - math.log(2.0)) < 1e-3


def test_head_refuses_bad_arguments():
    c = case(64)
    h, t = dev(c["h"][:2]), dev(c["t"][:2], torch.int32)
    out = torch.empty(2, device="cuda")
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    assert lib().loco_op_lm_head_nll(ptr(h), 768, ptr(c["dw"]), 768, ptr(t), 2, 64, IGNORE, ptr(out), ptr(small), 16, stream()) == -3
    assert lib().loco_op_lm_head_nll(ptr(h), 766, ptr(c["dw"]), 768, ptr(t), 2, 64, IGNORE, ptr(out), ptr(small), 1 << 20, stream()) == -1


# ---- gelu_new ---------------------------------------------------------------------------------------------------------------------
def gelu_new_ref64(x):
    """x / (1 + e^(-2u)), u = sqrt(2/pi) (x + 0.044715 x^3): HF's 0.5 x (1 + tanh u) without the 1 + tanh cancellation of the negative tail
    (tests/test_lm_ref.py checks that the two forms agree).  -inf gives NaN in both forms, as HF's own fp32 module does."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
        return x / (1.0 + np.exp(-2.0 * u)), np.abs(2.0 * u) / math.log(2.0)


def test_gelu_new_epilogue_on_hostile_values():
    """Bar, from the formula's own roundings.  u is formed with four fp32 roundings (0.044715 x, x x, the fma, the factor): 2^-22 relative.
    The exponent t = 2 log2(e) |u| of the exp2 then carries an absolute error of (2^-22 + 2^-24) t, i.e. a relative error of
    ln 2 x 1.25 x 2^-22 x t in e = 2^-t, which reaches the result x / (1 + e) multiplied by e / (1 + e) <= 1.  v_exp_f32 (1 ulp), the
    sum 1 + e and the division add at most 2^-23 + 2^-24 + 2^-24 = 2^-22.  Hence |err| <= 2^-22 (1.5 + 0.87 t) |ref|, with half of the
    first term to spare, plus one smallest normal number: below FLT_MIN no relative bar can hold (value_domain_cases.SUBNORMAL_QUANTUM
    makes the same allowance)."""
    grid, specials = vd.gelu_grid()
    extra = np.asarray([100.0, 1e3, 1e4, -100.0, -1e3, -1e4], F32)
    x = np.concatenate([specials, grid, extra]).astype(F32)
    width = 1024
    rows = -(-x.size // width)
    cols = np.ones(rows * width, F32)
    cols[:x.size] = x
    cols = cols.reshape(rows, width)
    M, K = 130, 32
    A, W = torch.zeros(M, K, device="cuda"), torch.zeros(width, K, device="cuda")
    got = []
    for row in cols:
        out = torch.full((M, width), -7.0, device="cuda")
        b = dev(row)
        check(lib().loco_op_gemm(ptr(A), K, ptr(W), K, ptr(b), None, width, ptr(out), width, M, width, K, 5, 1, 1, 0, 0, 0, 0, stream()), "gemm")
        torch.cuda.synchronize()
        v = out.view(torch.int32)
        assert bool((v == v[:1]).all())                       # every row of the tile computes the same bits
        got.append(out[0].double().cpu().numpy())
    got = np.stack(got).reshape(-1)[:x.size]
    ref, t = gelu_new_ref64(x)
    fin = np.isfinite(x)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        bar = 2.0 ** -22 * (1.5 + 0.87 * np.minimum(t, 300.0)) * np.abs(ref) + 2.0 ** -126
        ratio = np.where(fin, err / bar, 0.0)
    i = int(np.argmax(ratio))
    record_figure("gelu_new_value_domain", worst_ratio_to_bar=float(ratio[i]), at=float(x[i]), values=int(fin.sum()))
    print("gelu_new worst err / bar", ratio[i], "at", x[i], "got", got[i], "ref", ref[i])
    assert np.isfinite(got[fin]).all() and (ratio <= 1.0).all(), (x[i], got[i], ref[i])
    assert np.isposinf(got[np.isposinf(x)]).all() and np.isnan(got[np.isnan(x)]).all() and np.isnan(got[np.isneginf(x)]).all()
    assert (got[x == 0] == 0).all()
    big = fin & (np.abs(x) >= 100)
    assert (got[big & (x > 0)] == x[big & (x > 0)]).all() and (got[big & (x < 0)] == 0).all()      # tanh saturates to +-1 exactly


def test_gelu_new_leaves_the_other_epilogues_alone():
    rng = np.random.default_rng(3)
    A, W, b = dev(rng.standard_normal((130, 64)).astype(F32)), dev(rng.standard_normal((128, 64)).astype(F32)), dev(rng.standard_normal(128).astype(F32))
    outs = {}
    for epi in (0, 1, 5):
        out = torch.empty(130, 128, device="cuda")
        check(lib().loco_op_gemm(ptr(A), 64, ptr(W), 64, ptr(b), None, 128, ptr(out), 128, 130, 128, 64, epi, 1, 1, 0, 0, 0, 0, stream()), "gemm")
        torch.cuda.synchronize()
        outs[epi] = out.double().cpu().numpy()
    ref, _ = gelu_new_ref64(outs[0])
    assert np.abs(outs[5] - ref).max() < 1e-5 and np.abs(outs[1] - vd.gelu_ref64(outs[0])).max() < 1e-5
    assert lib().loco_op_gemm(ptr(A), 64, ptr(W), 64, ptr(b), None, 128, ptr(out), 128, 130, 128, 64, 6, 1, 1, 0, 0, 0, 0, stream()) < 0


# ---- embedding --------------------------------------------------------------------------------------------------------------------
def test_embed_ragged_windows_and_a_bad_id():
    V, S = 1003, 17
    rng = np.random.default_rng(5)
    wte, wpe = rng.standard_normal((V, 768)).astype(F32), rng.standard_normal((32, 768)).astype(F32)
    tokens = rng.integers(0, V, 60).astype(np.int32)
    starts, lens = np.asarray([0, 3, 40, 59, 10], np.int32), np.asarray([5, 17, 17, 1, 0], np.int32)   # overlapping windows, a full one, an empty one
    d_starts, d_lens, d_wte, d_wpe = dev(starts, torch.int32), dev(lens, torch.int32), dev(wte), dev(wpe)   # named: alive until the kernel has run

    def run(tok):
        x = torch.full((len(starts), S, 768), -7.0, device="cuda")
        status = torch.full((1,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        d_tok = dev(tok, torch.int32)
        check(lib().loco_op_lm_embed(ptr(d_tok), ptr(d_starts), ptr(d_lens), ptr(d_wte), V, ptr(d_wpe), ptr(x), len(starts), S, ptr(status), stream()),
              "lm_embed")
        torch.cuda.synchronize()
        return x.cpu().numpy(), int(status.item())

    def expect(tok):
        ref = np.zeros((len(starts), S, 768), F32)
        for b, (a, n) in enumerate(zip(starts, lens)):
            for s in range(n):
                if 0 <= tok[a + s] < V:
                    ref[b, s] = wte[tok[a + s]] + wpe[s]
        return ref
    x, status = run(tokens)
    assert status == 0x7F7F7F7F and np.array_equal(x, expect(tokens))     # one fp32 add: the same bits
    bad = tokens.copy()
    bad[44], bad[50], bad[58] = V, -3, V + 7                               # 44 and 50 lie in window 2; 58 in no window
    x, status = run(bad)
    assert status == 44 and np.array_equal(x, expect(bad))                 # the first bad position; its row embeds as zeros
