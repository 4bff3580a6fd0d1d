#!/usr/bin/env python3
"""Bit-for-bit comparison of the existing decoder entry points between two builds of this repository (a parent checkout and this
tree, each with its own libloco_asr.so): loco_decoder_generate (ids and step logits) and loco_decoder_begin + loco_decoder_step on
GENERATE["b7_len40_30s"], and loco_decoder_forward (logits and the 7 hidden states) on TEACHER_FORCED[3] of
tests/decoder_sweep_cases.py, 12 + 6 layers; then the model's Python surface (forward with labels and attentions, score, align, score_many,
align_many, generate_many, generate with scores) on the 2 + 2 layer model of the pool tests; then three operator-level blocks that reach
the rules the decoder's kernels share (csrc/decoder_common.h) on inputs the model never produces: loco_decoder_score's argmax path on
rows with ties, NaN and infinities, loco_op_decoder_attention beside loco_op_decoder_attention_probs around the tile and split
boundaries, and loco_decoder_pool_* with a free, a finishing and a full-length slot in one step.  One process per tree, since a process
loads one library:

    python tools/decoder_parent_compare.py dump PARENT_TREE out/parent
    python tools/decoder_parent_compare.py dump . out/new
    python tools/decoder_parent_compare.py compare out/parent out/new     # exits non-zero on any differing byte
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np


def dump(root, outdir):
    import torch
    root = os.path.abspath(root)
    os.makedirs(outdir, exist_ok=True)
    for p in (root, os.path.join(root, "tests")):
        sys.path.insert(0, p)
    la = importlib.import_module("loco-asr_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(la.__file__))) == root, la.__file__
    import decoder_sweep_cases as cases
    synth = la.synth
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = synth.split_state_dict(synth.encoder_state_dict(0))
    dec, post = synth.split_decoder_state_dict(synth.decoder_state_dict(13))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dec), postnet_state_dict=t(post)).to("cuda")
    save = lambda name, x: np.save(os.path.join(outdir, name + ".npy"), x.cpu().numpy())  # noqa: E731
    _, lengths_of, first_index, max_length = cases.GENERATE["b7_len40_30s"]
    x, m = synth.batch(lengths_of(synth), first_index=first_index)
    enc_out, frames = model._encode(torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda())
    ids, steps = model._decoder_runtime.generate(enc_out, frames, max_length, True)
    torch.cuda.synchronize()
    save("generate_ids", ids), save("generate_step_logits", steps), save("encoder_out", enc_out)
    lib, h = model.speecht5.encoder._lib, model.speecht5.encoder._handle
    B, T, S = enc_out.shape[0], enc_out.shape[1], 12
    need = lib.loco_decoder_workspace_bytes(h, B, T, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda tn: C.c_void_p(tn.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.loco_decoder_begin(h, p(enc_out), p(frames), B, T, S, p(ws), need, st) == 0
    lg = torch.empty((S - 1, B, 81), device="cuda")
    for step in range(S - 1):
        assert lib.loco_decoder_step(h, B, T, S, step, p(lg[step]), p(ws), need, st) == 0
    torch.cuda.synchronize()
    save("step_logits", lg)
    Bt, St, Tt, fr = cases.TEACHER_FORCED[3]
    e = (synth.hashed_uniform(f"dec_oracle/enc/{Bt}/{St}/{Tt}", (Bt, Tt, 768), 2) * np.float32(1.5)).astype(np.float32)
    tids = cases.teacher_forced_ids(synth, Bt, St)
    logits, hs = model._decoder_runtime.forward(torch.from_numpy(e).cuda(), torch.tensor(fr, dtype=torch.int32).cuda(),
                                                torch.from_numpy(tids).to(torch.int32).cuda(), True)
    torch.cuda.synchronize()
    save("forward_logits", logits), save("forward_hidden", torch.stack(hs))
    del model
    dump_ops(dump_small(la, save), save)
    print("dumped", sorted(os.listdir(outdir)), "from", root)


def dump_small(la, save):
    """The model's Python surface on the 2 + 2 layer model and six clips of tests/test_gpu_corpus_walk.py: forward with every
    output, score, align, their corpus forms, generate_many and generate with scores."""
    import torch
    import decoder_pool_cases as pc
    synth = la.synth
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = synth.split_state_dict(synth.encoder_state_dict(0, pc.ENC_LAYERS))
    dec, post = synth.split_decoder_state_dict(synth.decoder_state_dict(pc.DEC_SEED, layers=pc.DEC_LAYERS))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), layers=pc.ENC_LAYERS, decoder_state_dict=t(dec),
                                                              postnet_state_dict=t(post)).to("cuda")
    oc = pc.oracle_clips(synth)
    batches = [dict(input_values=torch.from_numpy(x).cuda(), attention_mask=torch.from_numpy(m).cuda()) for x, m in pc.pairs(synth, oc[0:4] + oc[10:12])]
    g = torch.Generator().manual_seed(3)
    labels = []
    for n in (5, 1, 9, 12, 2, 7):
        row = torch.randint(4, 81, (n,), generator=g)
        row[-1] = 2
        labels.append(row)
    b, lab = batches[1], torch.full((2, 12), -100)
    lab[0, :9], lab[1] = labels[2], labels[3]
    out = model(**b, labels=lab, output_attentions=True, output_hidden_states=True)
    for name in ("logits", "encoder_last_hidden_state", "loss", "token_logprobs"):
        save("small_forward_" + name, getattr(out, name))
    for name in ("decoder_hidden_states", "decoder_attentions", "cross_attentions", "encoder_attentions"):
        save("small_forward_" + name, torch.stack(getattr(out, name)))
    sc = model.score(**b, labels=lab)
    for name in ("token_logprobs", "sequence_logprob", "tokens", "loss"):
        save("small_score_" + name, getattr(sc, name))
    al = model.align(**b, labels=lab, return_attention=True)
    for name in ("start_frames", "end_frames", "start_times", "end_times", "attention"):
        save("small_align_" + name, getattr(al, name))
    for u, (lp, total) in enumerate(model.score_many(batches, labels, pack=2)):
        save(f"small_score_many_{u}_token_logprobs", lp), save(f"small_score_many_{u}_sum", total)
    for u, al in enumerate(model.align_many(batches, labels, pack=2, return_attention=True)):
        for name in ("start_frames", "end_frames", "start_times", "end_times", "attention"):
            save(f"small_align_many_{u}_{name}", getattr(al, name))
    ids, logits, scores = model.generate_many(batches, max_length=[3, 9, 2, 17, 5, 40], slots=3, return_logits=True, return_scores=True)
    for u in range(6):
        save(f"small_generate_many_{u}_ids", ids[u]), save(f"small_generate_many_{u}_logits", logits[u]), save(f"small_generate_many_{u}_scores", scores[u])
    gen = model.generate(**b, return_dict_in_generate=True, output_scores=True, max_length=12)
    save("small_generate_sequences", gen.sequences), save("small_generate_scores", torch.stack(gen.scores))
    save("small_generate_token_logprobs", gen.token_logprobs), save("small_generate_sequence_logprobs", gen.sequence_logprobs)
    save("small_generate_last_lengths", model._decoder_runtime.last_lengths)
    torch.cuda.synchronize()
    return model


def dump_ops(model, save):
    """Operator-level blocks: every one small, all inputs drawn from a seeded CPU generator."""
    import torch
    lib, h = model.speecht5.encoder._lib, model.speecht5.encoder._handle
    p = lambda tn: C.c_void_p(tn.data_ptr()) if tn is not None else None  # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    g = torch.Generator().manual_seed(29)
    inf, nan = float("inf"), float("nan")
    # loco_decoder_score with targets = NULL: the row's argmax and its log-probability.  V = 130: a lane holds up to three columns.
    for V in (1, 81, 130):
        base = torch.randn((8, V), generator=g)
        rows = [base[0].clone() for _ in range(8)]  # row 0: a plain row
        rows[1][:] = 0.75                           # all entries equal
        rows[2] = base[2].clamp(max=1.0)            # equal maxima at columns 5 and 70
        rows[3] = base[3].clone()                   # NaN at 3 and at 40
        rows[4] = base[4].clone()                   # NaN beside +inf
        rows[5][:] = -inf                           # all -inf
        rows[6] = base[6].clone()                   # +inf in the last column
        rows[7] = base[7].clone()                   # -inf but for one column
        for col, val in ((5, 2.5), (70, 2.5)):
            if col < V:
                rows[2][col] = val
        for col in (3, 40):
            if col < V:
                rows[3][col] = nan
        for col, val in ((9, inf), (10, nan), (11, inf)):
            if col < V:
                rows[4][col] = val
        rows[6][V - 1] = inf
        rows[7][:V - 1] = -inf
        x = torch.stack(rows).cuda()
        lp, ch = torch.empty(8, device="cuda"), torch.empty(8, dtype=torch.int32, device="cuda")
        sl, cnt, loss = torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, device="cuda")
        assert lib.loco_decoder_score(p(x), V, None, 1, 8, V, -100, p(lp), p(ch), p(sl), p(cnt), p(loss), st()) == 0
        torch.cuda.synchronize()
        for name, v in (("chosen", ch), ("logprob", lp), ("seq_logprob", sl), ("seq_count", cnt), ("loss", loss)):
            save(f"op_score_V{V}_{name}", v)
    # the attention and the probabilities kernel on the same q, k: tiles of 64 keys, two key splits at (Sq, Tk) = (1, 300)
    B = 2
    for Sq in (1, 3):
        for Tk in (1, 63, 64, 65, 300):
            q = torch.randn((B, Sq, 768), generator=g).cuda()
            k = torch.randn((B, Tk, 768), generator=g).cuda()
            v = torch.randn((B, Tk, 768), generator=g).cuda()
            need = int(lib.loco_decoder_attention_scratch_bytes(B, Sq, Tk))
            scr = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
            for ci, counts in enumerate(((0, Tk), (Tk - 1, 1))):
                kc = torch.tensor(counts, dtype=torch.int32).cuda()
                for causal in (0, 1):
                    tag = f"Sq{Sq}_Tk{Tk}_kc{ci}_c{causal}"
                    for off in sorted({0, max(Tk - Sq, 0)} if causal else {0}):
                        out = torch.empty((B, Sq, 768), device="cuda")
                        assert lib.loco_op_decoder_attention(p(q), p(k), p(v), p(kc), p(out), B, Sq, Tk, causal, off, 0.125, p(scr), scr.numel(), st()) == 0
                        save(f"op_attn_{tag}_off{off}", out)
                    P = torch.empty((B, 12, Sq, Tk), device="cuda")
                    assert lib.loco_op_decoder_attention_probs(p(q), p(k), p(kc), p(P), B, Sq, Tk, causal, 768, Sq * 768, 768, Tk * 768, 0.125, st()) == 0
                    save(f"op_probs_{tag}", P)
    # loco_decoder_pool_* on the 2-layer model
    T, S = 20, 8
    enc = torch.randn((3, T, 768), generator=g).cuda()

    def pool(tag, slots, admits):
        """admits: {step: (slot ids, clip of enc, rows, frames or None, caps)}; steps until no slot is open"""
        need = int(lib.loco_decoder_pool_workspace_bytes(h, slots, T, S))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        block = torch.zeros(4 + 2 * slots, dtype=torch.int32).pin_memory()
        toks = torch.zeros((slots, S), dtype=torch.int32).pin_memory()
        assert lib.loco_decoder_pool_init(h, slots, T, S, p(ws), need, st()) == 0
        logits, blocks = [], []
        for step in range(2 * S):
            if step in admits:
                ids, clip, rows, frames, caps = admits[step]
                n = len(ids)
                fr = torch.tensor(frames, dtype=torch.int32).cuda() if frames is not None else None
                assert lib.loco_decoder_pool_admit(h, slots, T, S, n, (C.c_int32 * n)(*ids), p(enc[clip]), T * 768, (C.c_int32 * n)(*rows), p(fr),
                                                   (C.c_int32 * n)(*caps), p(ws), need, st()) == 0
            lg = torch.empty((slots, 81), device="cuda")
            assert lib.loco_decoder_pool_step(h, slots, T, S, S - 2, T, p(lg), p(ws), need, st()) == 0
            assert lib.loco_decoder_pool_poll(h, slots, T, S, p(block), p(ws), need, st()) == 0
            torch.cuda.synchronize()
            logits.append(lg), blocks.append(block.clone())
            if int(block[0]) == 0 and step >= max(admits):
                break
        for r in range(slots):
            assert lib.loco_decoder_pool_read(h, slots, T, S, r, p(toks[r]), p(ws), need, st()) == 0
        torch.cuda.synchronize()
        lengths = blocks[-1][4 + slots:].tolist()
        for r in range(slots):
            toks[r, lengths[r]:] = -1  # beyond the utterance the buffer is the workspace's own
        save(f"op_pool_{tag}_logits", torch.stack(logits)), save(f"op_pool_{tag}_poll", torch.stack(blocks)), save(f"op_pool_{tag}_tokens", toks)

    pool("one_slot_cap2", 1, {0: ([0], 0, [T], None, [2])})
    # step 0 sees slot 0 finishing (cap 2), slot 1 free and slot 2 on its way to the full length; slot 1 is admitted while slot 2 goes on
    pool("three_slots", 3, {0: ([0, 2], 0, [T, 13], None, [2, S]), 1: ([1], 2, [T], [17], [4])})


def compare(a, b):
    ok = True
    for f in sorted(set(os.listdir(a)) | set(os.listdir(b))):
        if not (os.path.exists(os.path.join(a, f)) and os.path.exists(os.path.join(b, f))):
            print(f, "MISSING on one side")
            ok = False
            continue
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        print(f, x.shape, "bit-identical" if same else "DIFFERENT")
        ok = ok and same
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
