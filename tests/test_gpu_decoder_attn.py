"""-m gpu: the decoder's attention probabilities (csrc/decoder_probs.hip, forward(output_attentions=True)) and the token timestamps
built on them (align, align_many, transcribe --timestamps).

1. P_self / P_cross of loco_decoder_forward_attn against the float64 restatement (tests/decoder_attn_ref.py) on the same fp32 encoder
   output, at the project's bar for attention probabilities: 1e-5 max abs (tests/test_gpu_attentions.py TOL["f32"]); row sums likewise
2. exactness: masked / future entries == 0, logits and hidden states bitwise with and without the flag, junk beyond frames[b] unread
3. the probabilities operator on random q / k          4. the DTW operator: all-equal A and planted exact ties against the CPU DTW
5. loco_decoder_align: A at the 1e-5 bar, the path EXACTLY the CPU DTW of the device's A; invariants; a subset of heads
6. model.align / align_many / forward(output_attentions=True)          7. the CLI          8. error codes
"""
import importlib
import json

import numpy as np
import pytest
import torch

import decoder_attn_ref as ref
import decoder_pool_cases as pc
import decoder_sweep_cases as cases
from conftest import golden, record_figure
from test_gpu_decoder import decoder_forward, full_model
from test_gpu_decoder_oracle import decoder_sd, tf_inputs
from test_gpu_decoder_pool import batches_of, small_model

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_attentions.py TOL["f32"]: max abs of a probability against float64
PROB_CASES = [c for c in cases.TEACHER_FORCED[:9] if c[0] != 64]  # the eight shapes the sweep names, imported: (64, 7, 49) is not among them


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def g13_seed():
    return int(golden("g13_decoder.npz")["decoder_seed"])


_refs = {}


def reference(gu, seed, B, S, T, frames):
    """The float64 restatement of one case, computed once: (P_self per layer, P_cross per layer)."""
    key = (seed, B, S, T, None if frames is None else tuple(frames))
    if key not in _refs:
        enc, ids = tf_inputs(gu, B, S, T, frames)
        _, ps, pc_ = ref.forward_with_attentions(enc, frames, ids, decoder_sd(gu, seed))
        _refs[key] = (ps, pc_)
    return _refs[key]


def ready(gu, model):
    enc = model.speecht5.encoder
    enc._ensure_handle(torch.device("cuda", 0))
    enc._sync_weights(torch.device("cuda", 0), 8)
    return model._decoder_runtime


def dev_frames(gu, frames):
    return gu.dev(np.asarray(frames), torch.int32) if frames is not None else None


# ---- 1 + 2. probabilities of the teacher-forced pass ----------------------------------------------------------------------------------
def test_the_sweep_names_eight_cases():
    assert [c[:3] for c in PROB_CASES] == [(1, 1, 1), (2, 2, 64), (3, 65, 257), (5, 13, 1499), (1, 450, 149), (65, 3, 49), (2, 4, 8192), (1, 8, 29999)]
    assert PROB_CASES[4][3] is None and PROB_CASES[1][3] == [64, 63] and PROB_CASES[2][3] == [257, 256, 1] and PROB_CASES[6][3] == [8192, 4097]


@pytest.mark.parametrize("B,S,T,frames", PROB_CASES, ids=lambda v: str(v) if isinstance(v, int) else "f")
def test_probabilities_against_float64(gu, g13_seed, B, S, T, frames):
    enc, ids = tf_inputs(gu, B, S, T, frames)
    model = full_model(gu, seed=g13_seed)
    rt = ready(gu, model)
    enc_d, fr_d, ids_d = gu.dev(enc), dev_frames(gu, frames), gu.dev(ids, torch.int32)
    logits, hs, p_self, p_cross = rt.forward_attn(enc_d, fr_d, ids_d, True)
    logits0, hs0 = decoder_forward(gu, model, enc_d, fr_d, ids_d)
    torch.cuda.synchronize()
    assert len(p_self) == len(p_cross) == 6
    assert torch.equal(logits, logits0) and all(torch.equal(a, b) for a, b in zip(hs, hs0))  # the flag changes no bit of what was there
    want_self, want_cross = reference(gu, g13_seed, B, S, T, frames)
    worst = dict(self_max_abs=0.0, cross_max_abs=0.0, self_row_sum=0.0, cross_row_sum=0.0)
    future = torch.ones((S, S), dtype=torch.bool).triu(1)
    for l in range(6):
        ps, pc_ = p_self[l].cpu(), p_cross[l].cpu()
        assert ps.shape == (B, 12, S, S) and pc_.shape == (B, 12, S, T) and ps.dtype == pc_.dtype == torch.float32
        assert bool(torch.isfinite(ps).all()) and bool(torch.isfinite(pc_).all())
        assert bool((ps[:, :, future] == 0).all())  # future keys: exactly 0
        if frames is not None:
            for b, n in enumerate(frames):
                assert bool((pc_[b, :, :, n:] == 0).all())  # masked keys: exactly 0
        worst["self_max_abs"] = max(worst["self_max_abs"], float((ps.double() - want_self[l]).abs().max()))
        worst["cross_max_abs"] = max(worst["cross_max_abs"], float((pc_.double() - want_cross[l]).abs().max()))
        worst["self_row_sum"] = max(worst["self_row_sum"], float((ps.double().sum(-1) - 1).abs().max()))
        worst["cross_row_sum"] = max(worst["cross_row_sum"], float((pc_.double().sum(-1) - 1).abs().max()))
    record_figure("decoder_attn_probs_vs_float64", B=B, S=S, T_enc=T, frames=None if frames is None else frames[:8], bar=TOL, **worst)
    print(f"decoder probabilities B={B} S={S} T={T}: {worst}")
    assert max(worst.values()) <= TOL, worst


def test_junk_beyond_frames_is_never_read(gu, g13_seed):
    B, S, T, frames = cases.JUNK_CASE
    enc, ids = tf_inputs(gu, B, S, T, frames)
    rt = ready(gu, full_model(gu, seed=g13_seed))
    fr, idd = dev_frames(gu, frames), gu.dev(ids, torch.int32)
    clean = rt.forward_attn(gu.dev(enc), fr, idd)
    junk = enc.copy()
    for b, n in enumerate(frames):
        junk[b, n:] = 1e30
    dirty = rt.forward_attn(gu.dev(junk), fr, idd)
    torch.cuda.synchronize()
    assert torch.equal(clean[0], dirty[0])
    for a, b in zip(clean[2] + clean[3], dirty[2] + dirty[3]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


# ---- 3. the probabilities operator ------------------------------------------------------------------------------------------------------
def probs_op(gu, q, k, kcount, causal, ldk=768):
    """loco_op_decoder_attention_probs on host q [B,Sq,768], k [B,Tk,768]; k rows sit ldk floats apart on the device."""
    B, Sq, _ = q.shape
    Tk = k.shape[1]
    kd = torch.full((B, Tk, ldk), 1e30, device="cuda")
    kd[:, :, :768] = gu.dev(k)
    qd = gu.dev(q)
    P = torch.full((B, 12, Sq, Tk), -7.0, device="cuda")
    kc = gu.dev(np.asarray(kcount), torch.int32) if kcount is not None else None
    gu.check(gu.lib().loco_op_decoder_attention_probs(gu.ptr(qd), gu.ptr(kd), gu.ptr(kc), gu.ptr(P), B, Sq, Tk, int(causal), 768, Sq * 768, ldk, Tk * ldk,
                                                      0.125, gu.stream()), "decoder_attention_probs")
    torch.cuda.synchronize()
    return P.cpu()


def probs_ref(q, k, kcount, causal):
    B, Sq, _ = q.shape
    Tk = k.shape[1]
    qh = torch.as_tensor(q).double().view(B, Sq, 12, 64).transpose(1, 2) * 0.125
    kh = torch.as_tensor(k).double().view(B, Tk, 12, 64).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2)
    vis = torch.ones((B, 1, Sq, Tk), dtype=torch.bool)
    if kcount is not None:
        vis = vis & (torch.arange(Tk)[None, None, None, :] < torch.as_tensor(kcount)[:, None, None, None])
    if causal:
        vis = vis & (torch.arange(Tk)[None, None, None, :] <= torch.arange(Sq)[None, None, :, None])
    return torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1), vis.expand(B, 12, Sq, Tk)


@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 257])
def test_op_against_float64(gu, Tk):
    g = torch.Generator().manual_seed(Tk)
    B, Sq = 3, 5
    q, k = torch.randn((B, Sq, 768), generator=g) * 1.5, torch.randn((B, Tk, 768), generator=g)
    k[0, 0, :64] += 4.0  # an outlier key of head 0: the maximum is not in the last tile
    kcount = [Tk, max(1, Tk - 1), max(1, Tk // 2)]
    P = probs_op(gu, q.numpy(), k.numpy(), kcount, False, ldk=1536)
    want, vis = probs_ref(q, k, kcount, False)
    d, rs = float((P.double() - want).abs().max()), float((P.double().sum(-1) - 1).abs().max())
    assert bool((P[~vis] == 0).all())
    worst = dict(max_abs=d, row_sum=rs)
    if Tk > 1:  # the causal form on a square launch, null key counts
        qc = torch.randn((2, Tk, 768), generator=g)
        Pc = probs_op(gu, qc.numpy(), k[:2].numpy(), None, True)
        wc, vc = probs_ref(qc, k[:2], None, True)
        assert bool((Pc[~vc] == 0).all())
        worst.update(causal_max_abs=float((Pc.double() - wc).abs().max()), causal_row_sum=float((Pc.double().sum(-1) - 1).abs().max()))
    record_figure("decoder_attn_probs_op", Tk=Tk, bar=TOL, **worst)
    print("probabilities operator", Tk, worst)
    assert max(worst.values()) <= TOL, worst


# ---- 4. the DTW operator ----------------------------------------------------------------------------------------------------------------
def dtw_op(gu, A, counts, frames, ld=None):
    B, S, T = A.shape
    ld = ld or T
    Ad = torch.full((B, S, ld), 1e30, device="cuda")
    Ad[:, :, :T] = gu.dev(A)
    n = gu.dev(np.asarray(counts), torch.int32)
    fr = dev_frames(gu, frames)
    start = torch.full((B, S), -7, dtype=torch.int32, device="cuda")
    end = torch.full((B, S), -7, dtype=torch.int32, device="cuda")
    lib = gu.lib()
    ws = torch.zeros(int(lib.loco_dtw_align_workspace_bytes(B, S, T)), dtype=torch.uint8, device="cuda")
    gu.check(lib.loco_op_dtw_align(gu.ptr(Ad), ld, gu.ptr(n), gu.ptr(fr), B, S, T, gu.ptr(start), gu.ptr(end), gu.ptr(ws), gu.stream()), "dtw_align")
    torch.cuda.synchronize()
    return start.cpu().numpy(), end.cpu().numpy()


def check_invariants(start, end, counts, frames, T):
    for b, n in enumerate(counts):
        F = T if frames is None else frames[b]
        assert (start[b, n:] == -1).all() and (end[b, n:] == -1).all()
        if n:
            assert start[b, 0] == 0 and end[b, n - 1] == F and (start[b, :n] < end[b, :n]).all() and (np.diff(start[b, :n]) >= 0).all()
            assert (np.diff(end[b, :n]) >= 0).all() and (start[b, 1:n] >= end[b, :n - 1] - 1).all()  # a frame is shared by neighbours at most


def test_dtw_op_pins_the_tie_rule(gu):
    rng = np.random.default_rng(11)
    B, S, T = 6, 9, 13
    counts, frames = [9, 3, 0, 9, 1, 5], [13, 13, 13, 4, 13, 1]  # n < F, n > F, an empty row, one token, one frame
    for name, A in (("ones", np.ones((B, S, T), np.float32)), ("zeros", np.zeros((B, S, T), np.float32)),
                    ("halves", (np.round(rng.random((B, S, T)) * 2) / 2).astype(np.float32)),  # planted exact ties
                    ("random", rng.random((B, S, T)).astype(np.float32))):
        for ld in (T, T + 3):
            start, end = dtw_op(gu, A, counts, frames, ld)
            ws, we = ref.dtw_batch(A, counts, frames)
            assert (start == ws).all() and (end == we).all(), (name, ld, start, ws)
            check_invariants(start, end, counts, frames, T)
    s1, e1 = dtw_op(gu, np.ones((1, 3, 5), np.float32), [3], None)
    assert s1.tolist() == [[0, 4, 4]] and e1.tolist() == [[5, 5, 5]]  # -A: the longest path, (s-1,t) before (s,t-1)
    s0, e0 = dtw_op(gu, np.zeros((1, 3, 5), np.float32), [3], None)
    assert s0.tolist() == [[0, 3, 4]] and e0.tolist() == [[3, 4, 5]]  # every path ties: the diagonal first


# ---- 5. loco_decoder_align ---------------------------------------------------------------------------------------------------------------
ALIGN_CASES = {  # (B, S, T_enc, frames, counts, heads)
    "n1_F1": (1, 1, 1, [1], [1], None),
    "n1_F257": (3, 65, 257, [257, 256, 1], [1, 65, 40], None),           # (n, F) = (1, 257); n > F with a single frame
    "n450_F149": (1, 450, 149, None, [450], None),                        # n > F, the token cap, the null frame pointer
    "n65_F1499_ragged": (4, 65, 1499, [1499, 1, 700, 1024], [65, 30, 0, 17], None),  # a row of n_b = 0
    "heads_subset": (3, 65, 257, [257, 256, 1], [64, 2, 65], [(5, 11), (0, 3), (2, 7), (2, 0)]),
}


@pytest.mark.parametrize("name", list(ALIGN_CASES))
def test_align_against_the_cpu_dtw(gu, g13_seed, name):
    B, S, T, frames, counts, heads = ALIGN_CASES[name]
    dec = importlib.import_module("loco-asr_amd.decoder")
    enc, ids = tf_inputs(gu, B, S, T, frames)
    rt = ready(gu, full_model(gu, seed=g13_seed))
    arr, pairs = dec.check_alignment_heads(heads, 6)
    start, end, A = rt.align(gu.dev(enc), dev_frames(gu, frames), gu.dev(ids, torch.int32), gu.dev(np.asarray(counts), torch.int32), arr, pairs, True)
    start2, end2, none = rt.align(gu.dev(enc), dev_frames(gu, frames), gu.dev(ids, torch.int32), gu.dev(np.asarray(counts), torch.int32), arr, pairs)
    torch.cuda.synchronize()
    assert none is None and torch.equal(start, start2) and torch.equal(end, end2)  # A kept in the workspace: the same path
    A, start, end = A.cpu(), start.cpu().numpy(), end.cpu().numpy()
    want_A = ref.mean_attention(reference(gu, g13_seed, B, S, T, frames)[1], heads)
    d = float((A.double() - want_A).abs().max())
    ws, we = ref.dtw_batch(A.numpy(), counts, frames)  # the float64 recurrence on the device's own A: the identical path
    same = bool((start == ws).all() and (end == we).all())
    record_figure("decoder_align", case=name, B=B, S=S, T_enc=T, A_max_abs=d, bar=TOL, path_equals_cpu_dtw=same)
    print("align", name, "A max abs", d, "path equal", same)
    assert d <= TOL, d
    assert same, (start, ws, end, we)
    check_invariants(start, end, counts, frames, T)


# ---- 6. the model's calls ------------------------------------------------------------------------------------------------------------------
def pad_labels(rows):
    lab = torch.full((len(rows), max(len(r) for r in rows)), -100)
    for i, r in enumerate(rows):
        lab[i, :len(r)] = r
    return lab


def test_model_forward_align_and_align_many(gu):
    dec = importlib.import_module("loco-asr_amd.decoder")
    model = small_model(gu)
    oc = pc.oracle_clips(gu.la.synth)
    batches = batches_of(gu, oc[0:4] + oc[10:12])  # three reference pairs of unequal lengths
    g = torch.Generator().manual_seed(3)
    labels = []
    for n in (5, 1, 9, 12, 2, 7):
        row = torch.randint(4, 81, (n,), generator=g)
        row[-1] = 2
        labels.append(row)
    # forward(output_attentions=True): HF's fields and shapes, the other outputs bitwise
    b0, lab0 = batches[0], pad_labels(labels[0:2])
    out = model(**b0, labels=lab0, output_attentions=True, output_hidden_states=True)
    plain = model(**b0, labels=lab0, output_hidden_states=True)
    L = len(out.decoder_attentions)
    T0, S0 = out.encoder_last_hidden_state.shape[1], lab0.shape[1]
    assert L == len(out.cross_attentions) == pc.DEC_LAYERS and len(out.encoder_attentions) == pc.ENC_LAYERS
    assert all(a.shape == (2, 12, S0, S0) for a in out.decoder_attentions) and all(a.shape == (2, 12, S0, T0) for a in out.cross_attentions)
    assert all(a.shape == (2, 12, T0, T0) for a in out.encoder_attentions)
    assert torch.equal(out.logits, plain.logits) and torch.equal(out.loss, plain.loss) and torch.equal(out.encoder_last_hidden_state, plain.encoder_last_hidden_state)
    assert all(torch.equal(a, b) for a, b in zip(out.decoder_hidden_states, plain.decoder_hidden_states))
    assert plain.decoder_attentions is None and plain.cross_attentions is None and plain.encoder_attentions is None
    for flag in (None, False):
        assert model(**b0, labels=lab0, output_attentions=flag).cross_attentions is None
    # align: A is the mean of that pass's cross-attention, the path the CPU DTW of A, the times the frames x 20 ms
    al = model.align(**b0, labels=lab0, return_attention=True)
    frames0 = model.speecht5.encoder.last_frames.cpu().tolist()
    mean = torch.stack([a.cpu().double() for a in out.cross_attentions]).mean(dim=(0, 2))
    assert float((al.attention.cpu().double() - mean).abs().max()) <= 1e-6
    ws, we = ref.dtw_batch(al.attention.cpu().numpy(), [len(r) for r in labels[0:2]], frames0)
    assert (al.start_frames.cpu().numpy() == ws).all() and (al.end_frames.cpu().numpy() == we).all()
    assert al.start_frames.dtype == torch.int32 and al.start_times.dtype == torch.float32
    want_t = np.where(we < 0, -1.0, we * 0.02).astype(np.float32)
    assert np.allclose(al.end_times.cpu().numpy(), want_t, rtol=0, atol=1e-6)
    assert model.align(**b0, labels=lab0).attention is None
    # align_many against align per pair: the path bit for bit, A within the probabilities' bar
    per_pair = []
    for i, b in enumerate(batches):
        a = model.align(**b, labels=pad_labels(labels[2 * i:2 * i + 2]), return_attention=True)
        for j in range(2):
            n = len(labels[2 * i + j])
            per_pair.append((a.start_frames[j, :n].cpu(), a.end_frames[j, :n].cpu(), a.attention[j, :n].cpu().double()))
    worst = 0.0
    for pack in (1, 3):
        got = model.align_many(batches, labels, pack=pack, return_attention=True)
        assert len(got) == 6
        for u, a in enumerate(got):
            st, en, A = per_pair[u]
            T_own = A.shape[1]
            assert a.start_frames.shape == (len(labels[u]),) and a.start_frames.is_cuda
            d = float((a.attention[:, :T_own].cpu().double() - A).abs().max())
            worst = max(worst, d)
            print("align_many pack", pack, "utterance", u, "A max abs vs align", d)
            assert bool((a.attention[:, T_own:] == 0).all())
            assert torch.equal(a.start_frames.cpu(), st) and torch.equal(a.end_frames.cpu(), en), (pack, u)
            assert d <= TOL, d
    record_figure("decoder_align_many", A_max_abs_vs_align=worst, bar=TOL)


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------------
def test_transcribe_timestamps(gu, tmp_path, monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = small_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on; 2-layer weights keep it quick
    common = ["--random-init", "--synthetic", "4", "--synthetic-seconds", "1", "--max-length", "6"]
    paths = {k: tmp_path / f"{k}.jsonl" for k in ("loop", "pool", "loop_times", "pool_times")}
    assert tr.main(common + ["--out", str(paths["loop"])]) == 0
    assert tr.main(common + ["--slots", "4", "--out", str(paths["pool"])]) == 0
    assert tr.main(common + ["--timestamps", "--out", str(paths["loop_times"])]) == 0
    assert tr.main(common + ["--timestamps", "--slots", "4", "--out", str(paths["pool_times"])]) == 0
    plain = [json.loads(l) for l in paths["loop"].read_text().splitlines()]
    assert paths["pool"].read_text() == paths["loop"].read_text()
    samples = gu.la.synth.mixed_lengths(4, 16000)
    for k in ("loop_times", "pool_times"):
        recs = [json.loads(l) for l in paths[k].read_text().splitlines()]
        assert len(recs) == 4
        for r, p, n in zip(recs, plain, samples):
            assert sorted(r) == ["id", "token_ids", "token_times"]
            assert r["id"] == p["id"] and r["token_ids"] == p["token_ids"]  # without the flag: the same fields, the same values
            row = r["token_ids"]
            tokens = row.index(2, 1) + 1 if 2 in row[1:] else len(row)
            times = r["token_times"]
            assert len(times) == tokens - 1, (k, r)  # one pair per generated token
            assert times[0][0] == 0.0 and all(a < b for a, b in times) and all(0.0 <= a and b <= n / 16000 for a, b in times)
            assert all(x[0] <= y[0] and x[1] <= y[1] for x, y in zip(times, times[1:]))


# ---- 8. error codes ----------------------------------------------------------------------------------------------------------------------------
def test_cabi_error_codes(gu, g13_seed):
    lib = gu.lib()
    model = full_model(gu, seed=g13_seed)
    ready(gu, model)
    h = model.speecht5.encoder._handle
    B, T = 2, 9
    enc_out = torch.zeros((B, T, 768), device="cuda")
    ids = torch.full((B, 451), 5, dtype=torch.int32, device="cuda")
    logits = torch.zeros((B, 451, 81), device="cuda")
    n = torch.ones(B, dtype=torch.int32, device="cuda")
    out = torch.zeros((B, 451), dtype=torch.int32, device="cuda")
    need = int(lib.loco_decoder_align_workspace_bytes(h, B, T, 450))
    assert need > int(lib.loco_decoder_workspace_bytes(h, B, T, 450)) > 0 and lib.loco_decoder_align_workspace_bytes(h, B, T, 451) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st = gu.stream()
    p = gu.ptr
    assert lib.loco_decoder_forward_attn(h, p(enc_out), None, B, T, p(ids), 451, p(logits), None, None, None, p(ws), need, st) == -1
    assert b"450" in lib.loco_last_error()
    assert lib.loco_decoder_align(h, p(enc_out), None, B, T, p(ids), 451, p(n), None, 0, None, p(out), p(out), p(ws), need, st) == -1
    assert b"450" in lib.loco_last_error()
    assert lib.loco_decoder_align(h, p(enc_out), None, B, T, p(ids), 450, p(n), None, 0, None, p(out), p(out), p(ws), need - 1, st) == -3
    assert lib.loco_decoder_align(h, p(enc_out), None, B, T, p(ids), 450, None, None, 0, None, p(out), p(out), p(ws), need, st) == -1
    import ctypes as C
    bad = (C.c_int32 * 2)(6, 0)
    assert lib.loco_decoder_align(h, p(enc_out), None, B, T, p(ids), 450, p(n), bad, 1, None, p(out), p(out), p(ws), need, st) == -1
    assert b"layer 6" in lib.loco_last_error()
    null_layer = (C.c_void_p * 6)()
    assert lib.loco_decoder_forward_attn(h, p(enc_out), None, B, T, p(ids), 4, p(logits), None, null_layer, None, p(ws), need, st) == -1
    assert b"layer 0" in lib.loco_last_error()
    eo_model, _ = gu.model(layers=1)
    e1 = eo_model.speecht5.encoder
    x, m = gu.la.synth.batch([16000, 9600])
    y = e1(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32)).last_hidden_state
    assert lib.loco_decoder_align_workspace_bytes(e1._handle, 2, 49, 40) == 0
    assert lib.loco_decoder_forward_attn(e1._handle, p(y), None, 2, y.shape[1], p(ids), 40, p(logits), None, None, None, p(ws), need, st) == -2
    assert lib.loco_decoder_align(e1._handle, p(y), None, 2, y.shape[1], p(ids), 40, p(n), None, 0, None, p(out), p(out), p(ws), need, st) == -2
    assert b"decoder" in lib.loco_last_error()
    torch.cuda.synchronize()
