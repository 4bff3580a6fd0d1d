#!/usr/bin/env python3
"""Where should the residual of the encoder's two N = 768 GEMMs be added: in their epilogue, or in the LayerNorm behind them?

Times, at the flagship M = 47 968 and in ONE process, the launches of both arrangements as encoder_f16x3 makes them:
  out_proj / ffn2 through loco_op_gemm_f16x3_desc, once with kEpiResidual and the residual as fp16 hi/lo planes, once with kEpiNone;
  the LayerNorm over 47 968 x 768 (planes out, as between layers), plain and with the residual planes.
Every library given is measured in the same rounds, interleaved main / alt / alt / main (profiles/r03_attention_long_ab.txt: the first
variant of a round meets the colder clocks), median over the rounds.

    python3 tools/ln_residual_bench.py [other.so ...]      a library without loco_op_layernorm_f16x3_residual skips that row"""
import ctypes as C
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = importlib.import_module("loco-asr_amd._lib")
lib = L.load()
libs = [("main", lib)]
for a in sys.argv[1:]:
    if a.endswith(".so"):
        alt = C.CDLL(os.path.abspath(a))
        for name in ("loco_op_gemm_f16x3_desc", "loco_op_layernorm_f16x3", "loco_op_layernorm_f16x3_residual"):
            if hasattr(alt, name):
                getattr(alt, name).restype, getattr(alt, name).argtypes = L.SIGNATURES[name]
        libs.append((os.path.basename(a)[3:-3] if os.path.basename(a).startswith("lib") else os.path.basename(a)[:-3], alt))
ROUNDS = 9
M, D = 47968, 768
torch.manual_seed(0)
P = lambda t: t.data_ptr()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def planes(rows, cols, scale=1.0):
    v = torch.randn(rows, cols, device="cuda") * scale
    hi = v.half()
    return hi, (v - hi.float()).half()


gemms = {}
for name, K in (("out_proj", 768), ("ffn2", 3072)):
    ahi, alo = planes(M, K)
    whi, wlo = planes(D, K, 0.03)
    gemms[name] = (K, ahi, alo, whi, wlo)
bias = torch.randn(D, device="cuda")
rhi, rlo = planes(M, D)
x = torch.randn(M, D, device="cuda")
gamma, beta = torch.rand(D, device="cuda") + 0.5, torch.randn(D, device="cuda")
Cc = torch.empty(M, D, device="cuda")
yhi = torch.empty(M, D, device="cuda", dtype=torch.float16)
ylo = torch.empty_like(yhi)


def gemm(lb, name, epi):
    K, ahi, alo, whi, wlo = gemms[name]
    d = L.LocoGemmF16Desc()
    d.struct_size = C.sizeof(d)
    d.M, d.N, d.K, d.epilogue, d.nb1, d.nb2, d.terms, d.out_scale = M, D, K, epi, 1, 1, 3, 1.0
    d.Ahi, d.Alo, d.Whi, d.Wlo, d.bias, d.C = P(ahi), P(alo), P(whi), P(wlo), P(bias), P(Cc)
    d.lda = d.ldw = K
    d.ldc = d.ldr = D
    if epi == 2:
        d.Rhi, d.Rlo = P(rhi), P(rlo)
    return lambda: L.check(lb.loco_op_gemm_f16x3_desc(C.byref(d), st()))


def ln(lb, resid):
    if resid:
        return lambda: L.check(lb.loco_op_layernorm_f16x3_residual(P(Cc), P(rhi), P(rlo), P(gamma), P(beta), None, P(yhi), P(ylo), None, M, D, 1e-5, st()))
    return lambda: L.check(lb.loco_op_layernorm_f16x3(P(Cc), P(gamma), P(beta), None, P(yhi), P(ylo), None, M, D, 1e-5, st()))


rows = [("out_proj epi=residual", lambda lb: gemm(lb, "out_proj", 2)), ("out_proj epi=none", lambda lb: gemm(lb, "out_proj", 0)),
        ("ffn2 epi=residual", lambda lb: gemm(lb, "ffn2", 2)), ("ffn2 epi=none", lambda lb: gemm(lb, "ffn2", 0)),
        ("layernorm", lambda lb: ln(lb, False)), ("layernorm + residual", lambda lb: ln(lb, True))]
Cc.copy_(x)
order = libs + libs[1:][::-1] + (libs[:1] if len(libs) > 1 else [])  # main alt ... alt main
res = {}
for rnd in range(ROUNDS + 1):
    for rname, make in rows:
        for vname, lb in order:
            if "+ residual" in rname and not hasattr(lb, "loco_op_layernorm_f16x3_residual"):
                continue
            call = make(lb)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            call(); e0.record(); call(); call(); e1.record(); torch.cuda.synchronize()
            if rnd:
                res.setdefault((rname, vname), []).append(e0.elapsed_time(e1) / 2 * 1e3)
print(f"M = {M}, N = {D}; microseconds per launch, median (min .. max) of {ROUNDS} rounds, {len(order)} slots per round: "
      + " ".join(v for v, _ in order))
for rname, _ in rows:
    for vname, _ in libs:
        t = sorted(res.get((rname, vname), []))
        if t:
            print(f"{vname:12s} {rname:24s} {t[len(t) // 2]:8.1f}  ({t[0]:.1f} .. {t[-1]:.1f})")
med = lambda r, v="main": sorted(res[(r, v)])[len(res[(r, v)]) // 2]
if ("layernorm + residual", "main") in res:
    g = (med("out_proj epi=residual") - med("out_proj epi=none")) + (med("ffn2 epi=residual") - med("ffn2 epi=none"))
    l = med("layernorm + residual") - med("layernorm")
    print(f"main: per layer the two epilogues give up {g:.1f} us, the two LayerNorms take on {2 * l:.1f} us; x 12 layers = "
          f"{12 * (g - 2 * l) / 1e3:+.3f} ms per step in favour of the LayerNorm")
