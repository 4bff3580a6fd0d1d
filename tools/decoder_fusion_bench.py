#!/usr/bin/env python3
"""What n-gram shallow fusion costs in the beam step -> profiles/decoder_fusion_cost.json (tools, not bench.py; it sets no bar but one:
the step WITHOUT a model must cost what it cost before).  All 6 decoder layers, device events, medians, clocks as found.
  (i)   the beam step at 64 slots, K = 4 (16 groups), T_enc = 249 with nothing attached: this library against a build of the parent
        commit (--parent-lib: `make` in a worktree of the parent, the .so copied to tools/ab/libparent.so), one fresh process per run,
        the two alternated --runs times.  Each run: the median of 9 timings of --steps steps from admission.  Recorded: every run, both
        medians, the parent's spread (min .. max of its runs) and whether this library's median lies inside it.
  (ii)  the same step with an order-6 model of about 10^6 grams attached (trained on a seeded random corpus, so most of the pool's
        contexts are unseen and every candidate walks the whole chain: the longest path)
  (iii) loco_op_ngram_logprobs alone on 64 rows of 33 tokens of that corpus (contexts that were seen), 20 launches per timing
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, S, K = 64, 249, 450, 4


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    la = importlib.import_module("loco-asr_amd")
    _libmod = importlib.import_module("loco-asr_amd._lib")
    if os.environ.get("LOCO_ASR_LIB"):  # a build of the parent: it predates the entry points this change adds, which (i) does not call
        old = C.CDLL(os.environ["LOCO_ASR_LIB"])
        for name in [n for n in _libmod.SIGNATURES if not hasattr(old, n)]:
            del _libmod.SIGNATURES[name]
    dec = importlib.import_module("loco-asr_amd.decoder")
    p = lambda tn: C.c_void_p(tn.data_ptr()) if tn is not None else None  # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    i32 = lambda vs: (C.c_int32 * len(vs))(*vs)  # noqa: E731

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0, 1))
    dsd, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(0))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), layers=1, decoder_state_dict=t(dsd), postnet_state_dict=t(post)).to("cuda")
    lib, e = _libmod.load(), model.speecht5.encoder
    x = torch.from_numpy(la.synth.batch([16000])[0]).cuda()
    model.generate(x, torch.ones_like(x, dtype=torch.int32), max_length=4)  # loads the weights
    cfg = dec.check_beam_args(K)[2]
    block = torch.zeros(4 + 2 * B, dtype=torch.int32).pin_memory()
    res = {}
    lm = None
    if args.child == "lm":
        P = importlib.import_module("loco-asr_amd.ngram")
        rng = np.random.default_rng(11)
        seqs = [rng.integers(4, e._decoder_vocab, int(rng.integers(8, 17))).tolist() for _ in range(args.sentences)]
        lm = P.NgramLM.train(seqs, 6, e._decoder_vocab).to("cuda")
        res["grams"] = len(lm)
        need = int(lib.loco_decoder_beam_fusion_workspace_bytes(e._handle, B, T, S, K))
    else:
        need = int(lib.loco_decoder_beam_workspace_bytes(e._handle, B, T, S, K))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def run(enc_out, steps):
        G = B // K
        _libmod.check(lib.loco_decoder_pool_init(e._handle, B, T, S, p(ws), ws.numel(), st()))
        if lm is not None:
            _libmod.check(lib.loco_decoder_pool_attach_ngram(e._handle, B, T, S, lm.handle, 0.3, 0.0, p(ws), ws.numel()))
        _libmod.check(lib.loco_decoder_pool_admit_beams(e._handle, B, T, S, C.byref(cfg), G, i32(range(G)), p(enc_out), T * 768, i32([T] * G), None,
                                                        i32([S] * G), p(ws), ws.numel(), st()))
        torch.cuda.synchronize()
        ms = timed(lambda: [_libmod.check(lib.loco_decoder_pool_step_beam(e._handle, B, T, S, i, T, None, None, None, p(ws), ws.numel(), st()))
                            for i in range(steps)]) / steps
        _libmod.check(lib.loco_decoder_pool_poll(e._handle, B, T, S, p(block), p(ws), ws.numel(), st()))
        torch.cuda.synchronize()
        return ms, int(block[0])

    for seed in range(32):  # encoder rows that keep every slot open through the timed steps
        enc_out = torch.randn((B, T, 768), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
        if run(enc_out, args.steps)[1] == B:
            break
    else:
        sys.exit("no draw of encoder rows keeps every slot open")
    runs = [run(enc_out, args.steps)[0] for _ in range(9)]
    res.update(step_ms=statistics.median(runs), step_runs=runs, encoder_rows_seed=seed)
    if lm is not None:
        rows = torch.full((B, S), 1, dtype=torch.int32)
        for r in range(B):
            rows[r, 0] = 2
            rows[r, 1:33] = torch.tensor((seqs[r] * 5)[:32], dtype=torch.int32)
        rows, cur = rows.cuda(), torch.full((B,), 33, dtype=torch.int32, device="cuda")
        out = torch.empty((B, lm.vocab), dtype=torch.float64, device="cuda")
        once = lambda: [_libmod.check(lib.loco_op_ngram_logprobs(lm.handle, p(rows), S, S, p(cur), B, p(out), st())) for _ in range(20)]  # noqa: E731
        once()
        alone = [timed(once) / 20 for _ in range(9)]
        res.update(ngram_kernel_ms=statistics.median(alone), ngram_kernel_runs=alone)
    print("RESULT " + json.dumps(res), flush=True)
    return 0


def spawn(kind, args, lib=None):
    env = dict(os.environ)
    env.pop("LOCO_ASR_LIB", None)
    if lib:
        env["LOCO_ASR_LIB"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(args.steps), "--sentences", str(args.sentences)],
                         env=env, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["nolm", "lm"], default=None)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "ab", "libparent.so"))
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--sentences", type=int, default=26000, help="of the random corpus the order-6 model is trained on (about 10^6 grams)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_fusion_cost.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not os.path.exists(args.parent_lib):
        sys.exit(f"{args.parent_lib}: build the parent commit's library there first (see this file's head)")
    res = {"clock_state": "as found (not pinned)", "slots": B, "num_beams": K, "T_enc": T, "S_max": S, "steps_per_timing": args.steps,
           "timings_per_run": 9}
    parent, this = [], []
    for i in range(args.runs):
        parent.append(spawn("nolm", args, args.parent_lib))
        this.append(spawn("nolm", args))
        print(f"run {i}: parent {parent[-1]['step_ms']:.4f} ms, this {this[-1]['step_ms']:.4f} ms", flush=True)
    pm, tm = [r["step_ms"] for r in parent], [r["step_ms"] for r in this]
    res["no_lm_step_ms"] = dict(parent_runs=pm, this_runs=tm, parent_median=statistics.median(pm), this_median=statistics.median(tm),
                                parent_spread=[min(pm), max(pm)], this_median_inside_parent_spread=min(pm) <= statistics.median(tm) <= max(pm))
    fused = spawn("lm", args)
    res["fused"] = dict(order=6, grams=fused["grams"], lm_weight=0.3, step_ms=fused["step_ms"], step_runs=fused["step_runs"],
                        over_no_lm=fused["step_ms"] / statistics.median(tm), ngram_kernel_alone_ms=fused["ngram_kernel_ms"],
                        ngram_kernel_runs=fused["ngram_kernel_runs"], ngram_kernel_rows=B, ngram_kernel_tokens_per_row=33)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not res["no_lm_step_ms"]["this_median_inside_parent_spread"]:  # the one bar: written out, then failed
        print(f"the step without a model: {statistics.median(tm):.4f} ms is outside the parent's {min(pm):.4f} .. {max(pm):.4f} ms", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
