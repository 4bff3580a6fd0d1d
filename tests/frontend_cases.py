"""Inputs, fp64 references and bars of the waveform front end's per-element contract, shared by tests/test_frontend_ref.py (CPU) and
tests/test_gpu_frontend_contract.py.  torch on the CPU only; the bars are op_check's (normalize_bar, conv0_bar, pos_conv_bar), whose
docstring carries the counts.

Frame counts: exact integers, the Python floor-division chain.
Normaliser: ragged counts with NaN beyond n and a DC offset per row (one of 1000), and one row longer than the apply kernel's grid.
conv0: T0 in {1, 63, 64, 65, 129} (L = 5 T0 + 5 + r, r walking 0 .. 4: samples the conv never reads), T0 = 16385 (a thread's second
  trip in conv0_moments_kernel), t0_clip, and hostile clips.  Each clip of a batch is shorter than the launch's L and zero-padded,
  so statistics over the unpadded length are not the statistics over T0.
pos_conv: shapes around the 128-frame tile and the 64-frame halo, a table whose rows are all different, and one-hot weights that
  turn the conv into one exact product h[t + tap - 64].
Every restatement takes `sabotage`: the named defect a correct bar must catch (tests/test_frontend_ref.py).
"""
import functools
import importlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import op_check as oc
import value_domain_cases as vd

synth = importlib.import_module("loco-asr_amd.synth")

F32 = np.float32
CONV_K = (10, 3, 3, 3, 3, 2, 2)
CONV_S = (5, 2, 2, 2, 2, 2, 2)


def hu(key, shape, scale=1.0):
    return torch.from_numpy(synth.hashed_uniform(key, shape)) * scale


# ---- frame counts -----------------------------------------------------------------------------------------------------------------
def frames_ref(n, sabotage=None):
    """floor((n - k) / s) + 1 over the seven conv layers, Python's floor division (HF: torch.div(..., rounding_mode="floor"))"""
    for k, s in zip(CONV_K, CONV_S):
        d = n - k
        n = (int(d / s) if sabotage == "truncate" else d // s) + 1
    return n


SWEEP_L = 1200
UNALIGNED_L = 65541
UNALIGNED_LENGTHS = [65541, 65540, 32772, 32771, 9]


def sweep_mask():
    """[1201, 1200] int32, row b holds b ones"""
    return (torch.arange(SWEEP_L)[None] < torch.arange(SWEEP_L + 1)[:, None]).to(torch.int32)


def unaligned_masks():
    """(prefix masks, masks with holes and the same sums) [5, 65541] int32.  Two parts of 32772 and 32769 samples; with a 16-byte
    aligned allocation rows 1 .. 3 start off a 16-byte boundary, rows 0 and 4 on one with a one-element tail behind part 1's int4 loop."""
    L = UNALIGNED_L
    m = (torch.arange(L)[None] < torch.tensor(UNALIGNED_LENGTHS)[:, None]).to(torch.int32)
    holes = m.clone()
    holes[1] = 1
    holes[1, 12345] = 0                                   # 65540 ones, the last sample among them
    holes[2] = 0
    holes[2, 1::2] = 1                                    # 32770 ones at the odd samples ...
    holes[2, [0, L - 1]] = 1                              # ... and two more: 32772
    holes[4] = 0
    holes[4, [0, 3, 100, 32771, 32772, 65535, 65536, 65539, 65540]] = 1  # 9 ones on both sides of the part boundary and in the tail
    assert holes.sum(1).tolist() == UNALIGNED_LENGTHS
    return m, holes


# ---- normaliser -------------------------------------------------------------------------------------------------------------------
NORM_L = 1031
NORM_COUNTS = [0, 1, 2, 3, 5, 127, 128, 129, 511, 513, 1030, 1031]
NORM_DC = [0.0, 0.3, -0.2, 1000.0, 0.05, -3.0, 0.0, 7.5, -0.01, 2.0, -40.0, 0.125]
NORM_PAD = -7.0
NORM_LONG_L = 524288 + 300


def _norm_rows(L, counts, dcs, first):
    x = torch.full((len(counts), L), float("nan"))
    for b, (n, dc) in enumerate(zip(counts, dcs)):
        x[b, :n] = torch.from_numpy((synth.clip(first + b, max(n, 1))[:n] * F32(0.5 + 0.25 * b) + F32(dc)).astype(F32))
    return x


@functools.lru_cache(maxsize=None)
def norm_ragged():
    """x [12, 1031] fp32 with NaN at i >= n, mask int32"""
    x = _norm_rows(NORM_L, NORM_COUNTS, NORM_DC, 40)
    mask = (torch.arange(NORM_L)[None] < torch.tensor(NORM_COUNTS)[:, None]).to(torch.int32)
    return x, mask


@functools.lru_cache(maxsize=None)
def norm_full():
    """x [4, 1031] without padding: the mask-free form"""
    return _norm_rows(NORM_L, [NORM_L] * 4, [0.0, 1000.0, -0.5, 3.0], 60)


@functools.lru_cache(maxsize=None)
def norm_long():
    """x [1, 524588], n = L - 77 with a mask"""
    n = NORM_LONG_L - 77
    x = _norm_rows(NORM_LONG_L, [n], [0.25], 70)
    return x, (torch.arange(NORM_LONG_L)[None] < n).to(torch.int32)


def norm_reference(x, counts, pad=NORM_PAD):
    """fp64 two-pass reference: (ref [B, L] with pad at i >= n, bar [B, L], zero at i >= n where the value must be pad exactly,
    S [B, L] = rstd (|mean| + |x - mean|), the forward scale)"""
    B, L = x.shape
    ref = torch.full((B, L), float(pad), dtype=torch.float64)
    bar = torch.zeros(B, L, dtype=torch.float64)
    S = torch.zeros(B, L, dtype=torch.float64)
    for b, n in enumerate(counts):
        if n == 0:
            continue
        v = x[b, :n].double()
        mean = v.sum() / n
        var = ((v - mean) ** 2).sum() / n
        rstd = 1.0 / torch.sqrt(var + 1e-7)
        ref[b, :n] = (v - mean) * rstd
        bar[b, :n] = oc.normalize_bar(v, ref[b, :n], float(mean), float(var), float((v * v).sum() / n), float(rstd), n)
        S[b, :n] = rstd * (mean.abs() + (v - mean).abs())
    return ref, bar, S


def norm_restated(x, counts, pad=NORM_PAD, sabotage=None):
    """The operator in float32 with its statistics in fp64, rounded once (wav_norm_coeffs_kernel)."""
    B, L = x.shape
    out = torch.full((B, L), float(pad), dtype=torch.float32)
    for b, n in enumerate(counts):
        ns = min(n + 1, L) if sabotage == "n+1" else n
        v = x[b, :ns].double()
        mean = v.sum() / ns if ns > 0 else torch.tensor(0.0, dtype=torch.float64)
        var = ((v * v).sum() / ns - mean * mean).clamp_min(0.0) if ns > 0 else torch.tensor(0.0, dtype=torch.float64)
        if sabotage == "unbiased" and ns > 1:
            var = var * ns / (ns - 1)
        mean32, rstd32 = mean.float(), (1.0 / torch.sqrt(var + 1e-7)).float()
        out[b, :n] = (x[b, :n] - mean32) * rstd32
    return out


# ---- conv0 + GroupNorm + GELU -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv0_weights():
    """(w [512, 10], gn_w [512], gn_b [512]) fp32, the synthetic checkpoint's"""
    sd = synth.encoder_state_dict(0, layers=0)
    p = "prenet.feature_encoder.conv_layers.0."
    return (torch.from_numpy(sd[p + "conv.weight"]).reshape(512, 10).contiguous(), torch.from_numpy(sd[p + "layer_norm.weight"]),
            torch.from_numpy(sd[p + "layer_norm.bias"]))


CONV0_SMALL_T0 = [1, 63, 64, 65, 129]
CONV0_LARGE_T0 = 16385
CONV0_CLIP = [129, 70, 1]
CONV0_HOSTILE = ["silence", "constant", "dc", "square", "impulse"]


def conv0_len(T0, r=0):
    return 5 * T0 + 5 + r


def _clips(L, lengths, first, scales):
    x = torch.zeros(len(lengths), L)
    for b, (n, s) in enumerate(zip(lengths, scales)):
        x[b, :n] = torch.from_numpy(synth.clip(first + b, n) * F32(s))
    return x


@functools.lru_cache(maxsize=None)
def conv0_input(name):
    """(x [B, L] fp32, unpadded lengths) of a named case: "small<T0>", "large", "clip", or a hostile clip's name"""
    if name.startswith("small"):
        T0 = int(name[5:])
        L = conv0_len(T0, CONV0_SMALL_T0.index(T0))
        lengths = [L, max(10, (2 * L) // 3), max(10, L // 3 + 1)]
        return _clips(L, lengths, 80 + T0, (1.0, 0.05, 7.0)), lengths
    if name == "large":
        L = conv0_len(CONV0_LARGE_T0)
        return _clips(L, [L - 4000], 90, (1.0,)), [L - 4000]
    if name == "clip":
        L = conv0_len(CONV0_CLIP[0])
        return _clips(L, [L, L, L], 95, (1.0, 0.3, 2.0)), [L, L, L]
    L = 8000
    if name == "silence":
        x = torch.zeros(1, L)
    elif name == "constant":
        x = torch.full((1, L), 0.75)
    elif name == "dc":
        x = torch.from_numpy(synth.clip(97, L) / np.abs(synth.clip(97, L)).max() + F32(5.0))[None]
    elif name == "square":
        x = torch.where((torch.arange(L) // 7) % 2 == 0, 1.0, -1.0)[None]
    elif name == "impulse":
        x = torch.zeros(1, L)
        x[0, 4003] = 1.0
    else:
        raise KeyError(name)
    return x.float().contiguous(), [L]


def conv0_windows(x, T0, start=0):
    """[B, T0, 10]: window t is x[5 t + start : 5 t + start + 10]"""
    return x[:, start:].unfold(1, 10, 5)[:, :T0]


def conv0_reference(x, t0_clip=None):
    """fp64, two-pass statistics over the launch's T0 frames, or over t0_clip[b] with zeros at and beyond it.
    -> (ref [B, T0, 512], bar, S = the recorded forward scale)"""
    w, gw, gb = (t.double() for t in conv0_weights())
    B, L = x.shape
    T0 = (L - 10) // 5 + 1
    win = conv0_windows(x.double(), T0)
    y = win @ w.T                                   # [B, T0, 512]
    Y = win.abs() @ w.abs().T
    tn = torch.tensor([T0] * B if t0_clip is None else t0_clip)
    live = (torch.arange(T0)[None] < tn[:, None])[:, :, None].double()
    cnt = tn.double()[:, None, None]
    mu = (y * live).sum(1, keepdim=True) / cnt
    var = (((y - mu) ** 2) * live).sum(1, keepdim=True) / cnt
    EY2 = ((Y * Y) * live).sum(1, keepdim=True) / cnt
    sc = gw / torch.sqrt(var + 1e-5)
    h = (y - mu) * sc + gb
    ref = oc.gelu64(h) * live
    bar = oc.conv0_bar(ref, h, y, Y, mu, sc, var, EY2, tn[:, None, None]) * live
    return ref, bar, sc.abs() * (Y + mu.abs()) + gb.abs()


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def conv0_restated(x, lengths=None, sabotage=None):
    """The operator in float32: the chain of 10 fmaf, fp64 statistics rounded once, fma(y - mu, sc, be), the kernel's GELU polynomial."""
    w, gw, gb = conv0_weights()
    B, L = x.shape
    T0 = (L - 10) // 5 + 1
    win = conv0_windows(x, T0, 1 if sabotage == "window+1" else 0)
    if win.shape[1] < T0:  # the shifted last window would leave the clip: repeat the one before
        win = torch.cat([win, win[:, -1:]], 1)
    y = torch.zeros(B, T0, 512)
    for k in range(10):
        y = _fma32(win[:, :, k, None], w[None, None, :, k], y)
    y64 = conv0_windows(x.double(), T0) @ w.double().T
    tn = torch.tensor([T0] * B)
    if sabotage == "unpadded":
        tn = torch.tensor([(n - 10) // 5 + 1 for n in lengths])
    elif sabotage == "T0-1":
        tn = torch.tensor([max(T0 - 1, 1)] * B)
    live = (torch.arange(T0)[None] < tn[:, None])[:, :, None].double()
    cnt = tn.double()[:, None, None]
    mean = (y64 * live).sum(1, keepdim=True) / cnt
    var = ((y64 * y64 * live).sum(1, keepdim=True) / cnt - mean * mean).clamp_min(0.0)
    mu32, sc32 = mean.float(), (gw.double() / torch.sqrt(var + 1e-5)).float()
    h = _fma32(y - mu32, sc32, gb[None, None].expand_as(y))
    return torch.from_numpy(vd.gelu_restated32(h.numpy()))


# ---- positional conv, fp32 --------------------------------------------------------------------------------------------------------
POS_SHAPES = [(1, 1, None), (2, 64, [64, 1]), (1, 129, None), (3, 193, [193, 128, 65]), (2, 257, [257, 129])]
SHIFT_TAPS = [0, 1, 63, 64, 65, 126, 127]
SHIFT_T = [129, 257]


@functools.lru_cache(maxsize=None)
def pos_weights32():
    """(folded weight [768, 48, 128] (out, in, tap), bias [768]) fp32: w = g v / ||v|| per tap (weight_norm, dim = 2)"""
    sd = synth.encoder_state_dict(0, layers=0)
    n = "prenet.pos_conv_embed.conv."
    g = torch.from_numpy(sd[n + "parametrizations.weight.original0"])
    v = torch.from_numpy(sd[n + "parametrizations.weight.original1"])
    return (v * (g / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True)))).contiguous(), torch.from_numpy(sd[n + "bias"])


def fold(w):
    """[768, 48, 128] (out, in, tap) -> the operator's [16][128][48][48] (group, tap, out, in)"""
    return w.view(16, 48, 48, 128).permute(0, 3, 1, 2).contiguous()


def one_hot_weight(tap, value=1.0):
    """[768, 48, 128]: w[48 g + o, o, tap] = value, everything else 0"""
    w = torch.zeros(768, 48, 128)
    o = torch.arange(768)
    w[o, o % 48, tap] = value
    return w


@functools.lru_cache(maxsize=None)
def pos_input(B, T, fp16_exact=False):
    """(h [B, T, 768], table [T + 2, 768] with all rows different)"""
    h = hu(f"fe.pos.h.{B}.{T}", (B, T, 768), 1.5)
    if fp16_exact:
        h = h.half().float()
    tab = hu(f"fe.pos.tab.{T}", (T + 2, 768), 1.0)
    return h, tab


def positions(B, T, frames, sabotage=None):
    fr = torch.full((B,), T) if frames is None else torch.tensor(frames)
    t = torch.arange(T)[None]
    valid = t < (fr[:, None] - (1 if sabotage == "pad_last" else 0))
    return torch.where(valid, t + (1 if sabotage == "pos+1" else 2), torch.ones_like(t))


def _pos_conv(h, w, bias, sabotage=None):
    """[B, T, 768] -> conv [B, T, 768] in h's dtype: Conv1d(k = 128, padding 64, 16 groups), the last of the T + 1 frames dropped"""
    B, T, _ = h.shape
    x = h.transpose(1, 2)
    if sabotage == "group":
        x = x.reshape(B, 16, 48, T).roll(1, 1).reshape(B, 768, T)
    full = F.conv1d(x, w, bias, padding=64, groups=16)            # [B, 768, T + 1]
    if sabotage == "tap+1":
        return full[:, :, 1:].transpose(1, 2)
    if sabotage == "no_drop":  # T + 1 frames per clip written back to back, read at T per clip: clip b starts b frames early
        flat = full.transpose(1, 2).reshape(B * (T + 1), 768)
        return flat[:B * T].reshape(B, T, 768)
    return full[:, :, :-1].transpose(1, 2)


def pos_reference(h, w, bias, tab, frames, count=oc.pos_conv_count):
    """fp64 -> (ref, bar, S of the whole expression)"""
    B, T, _ = h.shape
    h64, w64, b64, tab64 = h.double(), w.double(), bias.double(), tab.double()
    pre = _pos_conv(h64, w64, b64)
    S = _pos_conv(h64.abs(), w64.abs(), b64.abs())
    g = oc.gelu64(pre)
    t = tab64[positions(B, T, frames)]
    return h64 + g + t, oc.pos_conv_bar(g, pre, S, h64, t, count), S + h64.abs() + t.abs()


def pos_restated(h, w, bias, tab, frames, sabotage=None):
    """float32: torch's conv, the kernel's GELU polynomial, hv + gelu + table in the kernel's order"""
    B, T, _ = h.shape
    pre = _pos_conv(h, w, bias, sabotage)
    g = torch.from_numpy(vd.gelu_restated32(pre.contiguous().numpy()))
    return h + g + tab[positions(B, T, frames, sabotage)]


def first_over(out, ref, bar):
    """index of the first element that is not within its bar (a NaN is not), or None"""
    bad = ~((out.double() - ref).abs() <= bar)
    if not bool(bad.any()):
        return None
    return tuple(int(i) for i in np.unravel_index(int(torch.nonzero(bad.reshape(-1))[0]), tuple(ref.shape)))
