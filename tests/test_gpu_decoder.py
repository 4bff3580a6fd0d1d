"""-m gpu: the SpeechT5 text decoder (csrc/decoder.hip, loco_decoder_*) against HuggingFace's outputs in
tests/golden/g13_decoder.npz (tests/golden/make_decoder_goldens.py) and against float64 torch-CPU evaluations written here."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from conftest import golden, record_figure

pytestmark = pytest.mark.gpu

BAR = 2e-5       # relative L2 vs HF fp32: the bar of every first-family golden in this suite
BAR_GEMM = 5e-6  # the loosest bar tests/test_gpu_ops.py holds a GEMM-class operator to
BAR_ATTN = 1e-5  # ... and an attention-class operator


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def g13():
    return golden("g13_decoder.npz")


_models = {}


def full_model(gu, precision="f16x3", seed=None):
    la = gu.la
    g = golden("g13_decoder.npz")
    seed = int(g["decoder_seed"]) if seed is None else seed
    if seed not in _models:
        sd = la.synth.encoder_state_dict(0)
        pre, enc = la.synth.split_state_dict(sd)
        dec, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(seed))
        t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
        _models[seed] = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dec), postnet_state_dict=t(post)).to("cuda")
    m = _models[seed]
    m.speecht5.encoder.precision = precision
    return m


def decoder_forward(gu, model, enc_out, frames, ids, hidden=True):
    enc = model.speecht5.encoder
    enc._ensure_handle(torch.device("cuda", 0))
    enc._sync_weights(torch.device("cuda", 0), 8)
    return model._decoder_runtime.forward(enc_out, frames, ids, hidden)


# ---- 1. golden B: the decoder alone ----------------------------------------------------------------------------------------
def test_decoder_forward_golden_b(gu, g13):
    la = gu.la
    enc_np = (la.synth.hashed_uniform("g13/enc", (3, 149, 768), 0) * np.float32(1.5)).astype(np.float32)
    ids = gu.dev(g13["b_ids"], torch.int32)
    frames = gu.dev(np.asarray([149, 97, 1]), torch.int32)
    model = full_model(gu)
    enc_out = gu.dev(enc_np)
    logits, hs = decoder_forward(gu, model, enc_out, frames, ids)
    torch.cuda.synchronize()
    r32, r64 = gu.rel_l2(logits, g13["b_logits32"]), gu.rel_l2(logits, g13["b_logits64"])
    probe = [5, 12, 23]  # B_PROBE_POS of the generator
    h = torch.stack([x[:, probe] for x in hs]).cpu()
    rh = [gu.rel_l2(h[l], g13["b_hidden32"][l]) for l in range(7)]
    rh64 = [gu.rel_l2(h[l], g13["b_hidden64"][l]) for l in range(7)]
    record_figure("decoder_forward_golden_b", logits_vs_hf32=r32, logits_vs_f64=r64, hidden_vs_hf32=rh, hidden_vs_f64=rh64)
    print("golden B: logits", r32, r64, "hidden", rh)
    assert r32 <= BAR, r32
    assert max(rh) <= BAR, rh
    # rows of enc_out at and beyond frames[b] are never read as keys
    junk = enc_out.clone()
    junk[1, 97:] = 1e30
    junk[2, 1:] = 1e30
    logits2, _ = decoder_forward(gu, model, junk, frames, ids, hidden=False)
    torch.cuda.synchronize()
    assert torch.equal(logits, logits2)


# ---- 2. golden A end to end ------------------------------------------------------------------------------------------------
def _a_inputs(gu, g13):
    x, m = gu.la.synth.batch([48000, 30400], first_index=int(g13["a_first_index"]))
    return gu.dev(x), gu.dev(m, torch.int32)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_golden_a_end_to_end(gu, g13, precision):
    model = full_model(gu, precision)
    x, m = _a_inputs(gu, g13)
    ids_hf = torch.from_numpy(g13["a_ids"])
    out = model(input_values=x, attention_mask=m, decoder_input_ids=ids_hf.to("cuda"))
    r = gu.rel_l2(out.logits, g13["a_logits32"])
    record_figure("decoder_golden_a_logits", precision=precision, vs_hf32=r, vs_f64=gu.rel_l2(out.logits, g13["a_logits64"]))
    print("golden A logits", precision, r)
    assert out.encoder_last_hidden_state.shape[0] == 2
    ids = model.generate(input_values=x, attention_mask=m, max_length=40)
    assert ids.dtype == torch.long and ids.is_cuda
    ids_def = model.generate(input_values=x, attention_mask=m)
    print("generate:", ids.cpu().tolist(), "hf:", ids_hf.tolist())
    assert r <= BAR, r
    assert ids.cpu().tolist() == ids_hf.tolist()
    assert ids_def.cpu().tolist() == g13["a_default_ids"].tolist()


def test_generate_stops_when_every_row_has_finished(gu, g13):
    """Golden C: with these weights every row emits </s>, HF returns S_c < 40 columns.  generate enqueues steps past that point (it
    looks at the device's open-rows word every 8 steps), must then take the early exit and trim to HF's length."""
    model = full_model(gu, seed=int(g13["decoder_seed_c"]))
    x, m = _a_inputs(gu, g13)
    want = torch.from_numpy(g13["c_ids"])
    assert want.shape[1] < 40
    ids, steps = model.generate(input_values=x, attention_mask=m, max_length=40, return_logits=True)
    assert ids.cpu().tolist() == want.tolist() and steps.shape[0] == want.shape[1] - 1
    assert model._decoder_runtime.last_lengths.tolist() == [int((r[1:] == 2).nonzero()[0]) + 2 for r in want]
    # the loop really stopped early: the device's step counter is well short of max_length - 1
    enc = model.speecht5.encoder
    ids450 = model.generate(input_values=x, attention_mask=m, max_length=450)
    assert ids450.cpu().tolist() == want.tolist()
    lib = gu.lib()
    B, T = 2, int(lib.loco_output_frames(x.shape[1]))
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = model._decoder_runtime._workspace
    state.copy_(ws[:16].view(torch.int32))  # the plan's first carve-out: [rows still open, steps completed]
    assert state.tolist()[0] == 0 and state.tolist()[1] == 8, state.tolist()


# ---- 3. step path vs teacher-forced path, determinism ------------------------------------------------------------------------
def test_step_vs_teacher_forced_and_determinism(gu, g13):
    model = full_model(gu)
    x, m = _a_inputs(gu, g13)
    ids, steps = model.generate(input_values=x, attention_mask=m, max_length=40, return_logits=True)
    ids2, steps2 = model.generate(input_values=x, attention_mask=m, max_length=40, return_logits=True)
    assert torch.equal(ids, ids2) and torch.equal(steps, steps2)
    tf = model(input_values=x, attention_mask=m, decoder_input_ids=ids).logits  # [B, S, V]
    a, b = steps.permute(1, 0, 2), tf[:, :-1]
    r = gu.rel_l2(a, b)
    rs = gu.rel_l2(steps, g13["a_step_logits32"][:steps.shape[0]])
    record_figure("decoder_step_vs_teacher_forced", rel_l2=r, step_logits_vs_hf32=rs, hf_cached_vs_uncached_rel_l2=float(g13["a_cached_vs_uncached"]))
    print("step vs teacher-forced", r, "step logits vs HF", rs)
    assert r <= BAR, r


# ---- 4. shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,max_length", [(1, 12), (33, 12), (2, 450)])
def test_generate_shapes(gu, B, max_length):
    model = full_model(gu)
    x, m = gu.la.synth.batch([16000 + 800 * (i % 5) for i in range(B)])
    ids, steps = model.generate(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32), max_length=max_length, return_logits=True)
    S = ids.shape[1]
    assert ids.shape[0] == B and 2 <= S <= max_length and bool((ids[:, 0] == 2).all())
    assert bool(torch.isfinite(steps).all())
    ids_c = ids.cpu()
    for b in range(B):  # argmax of the step's logits until </s>, <pad> after it
        done = False
        for t in range(S - 1):
            want = 1 if done else int(torch.argmax(steps[t, b]))
            assert int(ids_c[b, t + 1]) == want, (b, t)
            done = done or want == 2
    if S < max_length:
        assert bool((ids_c == 2)[:, 1:].any(dim=1).all())  # early stop only when every row has finished
    # the step path against the teacher-forced pass on the ids it produced (max_length 450: the step's self-attention runs with two
    # key splits from t = 256 on; both paths place <pad> tokens at the zero position row, so finished rows agree too)
    tf = model(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32), decoder_input_ids=ids).logits
    r = gu.rel_l2(steps.permute(1, 0, 2), tf[:, :-1])
    record_figure("decoder_generate_shapes", B=B, max_length=max_length, S=S, step_vs_teacher_forced=r)
    assert r <= BAR, r


def test_batch_above_cap(gu):
    """B above the weight-streaming GEMM's 64 rows: generate refuses by name (split the batch); the teacher-forced pass has no cap."""
    model = full_model(gu)
    x, m = gu.la.synth.batch([8000] * 65)
    with pytest.raises(ValueError, match="64"):
        model.generate(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32), max_length=4)
    ids = torch.full((65, 3), 5, dtype=torch.long, device="cuda")
    assert model(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32), decoder_input_ids=ids).logits.shape == (65, 3, 81)
    lib = gu.lib()
    a = torch.zeros((65, 768), device="cuda")
    assert lib.loco_op_skinny_gemm(gu.ptr(a), 768, gu.ptr(a), 768, None, None, 0, gu.ptr(a), 768, 65, 8, 768, 0, gu.stream()) == -1
    assert b"64" in lib.loco_last_error()


# ---- 5. operators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("M", [1, 2, 3, 17, 63, 64])  # 3 and 63: M mod 4 = 3, the remainder of the 4-row register pass
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_op_skinny_gemm(gu, M, K, epi):
    N = {768: 2304, 3072: 81}[K] if epi != 1 else 3072 if K == 768 else 768
    hu = gu.la.synth.hashed_uniform
    A = hu(f"sg/A/{M}/{K}", (M, K), 3) * np.float32(1.7)
    W = hu(f"sg/W/{N}/{K}", (N, K), 3) * np.float32(2.0 / np.sqrt(K))
    bias = hu(f"sg/b/{N}", (N,), 3) * np.float32(0.3)
    R = hu(f"sg/R/{M}/{N}", (M, N), 3)
    ref = torch.from_numpy(A).double() @ torch.from_numpy(W).double().T + torch.from_numpy(bias).double()
    if epi == 1:
        ref = torch.nn.functional.gelu(ref)
    if epi == 2:
        ref = ref + torch.from_numpy(R).double()
    a, w, b_, r_ = gu.dev(A), gu.dev(W), gu.dev(bias), gu.dev(R)
    c = torch.full((M, N), float("nan"), device="cuda")
    gu.check(gu.lib().loco_op_skinny_gemm(gu.ptr(a), K, gu.ptr(w), K, gu.ptr(b_), gu.ptr(r_) if epi == 2 else None, N, gu.ptr(c), N, M, N, K, epi,
                                          gu.stream()), "skinny_gemm")
    torch.cuda.synchronize()
    r = gu.rel_l2(c, ref)
    record_figure("op_skinny_gemm", M=M, N=N, K=K, epilogue=epi, rel_l2=r)
    assert r <= BAR_GEMM, r


@pytest.mark.parametrize("M,K,epi", [(63, 768, 2), (3, 3072, 2), (17, 768, 1)])
def test_op_skinny_gemm_strided(gu, M, K, epi):
    """Row strides wider than the rows (lda > K, ldr > N, ldc > N): the gap columns of A and R hold values that would show in the
    result if read, the gap columns of C a sentinel that must stay."""
    N = 81 if K == 3072 else 2304
    lda, ldr, ldc = K + 8, N + 5, N + 7  # lda stays a multiple of 4 floats (the kernel's 16-byte loads)
    hu = gu.la.synth.hashed_uniform
    A = hu(f"sgs/A/{M}/{K}", (M, lda), 3) * np.float32(1.7)
    W = hu(f"sgs/W/{N}/{K}", (N, K), 3) * np.float32(2.0 / np.sqrt(K))
    bias = hu(f"sgs/b/{N}", (N,), 3) * np.float32(0.3)
    R = hu(f"sgs/R/{M}/{N}", (M, ldr), 3)
    ref = torch.from_numpy(A[:, :K]).double() @ torch.from_numpy(W).double().T + torch.from_numpy(bias).double()
    if epi == 1:
        ref = torch.nn.functional.gelu(ref)
    if epi == 2:
        ref = ref + torch.from_numpy(R[:, :N]).double()
    a, w, b_, r_ = gu.dev(A), gu.dev(W), gu.dev(bias), gu.dev(R)
    sentinel = -12345.5
    c = torch.full((M, ldc), sentinel, device="cuda")
    gu.check(gu.lib().loco_op_skinny_gemm(gu.ptr(a), lda, gu.ptr(w), K, gu.ptr(b_), gu.ptr(r_) if epi == 2 else None, ldr, gu.ptr(c), ldc, M, N, K, epi,
                                          gu.stream()), "skinny_gemm")
    torch.cuda.synchronize()
    r = gu.rel_l2(c[:, :N], ref)
    record_figure("op_skinny_gemm_strided", M=M, N=N, K=K, epilogue=epi, lda=lda, ldr=ldr, ldc=ldc, rel_l2=r)
    assert r <= BAR_GEMM, r
    assert bool((c[:, N:] == sentinel).all())


def _attn_ref(q, k, v, counts, causal, offset, scale):
    B, Sq, _ = q.shape
    Tk = k.shape[1]
    qh, kh, vh = (t.double().view(B, -1, 12, 64).transpose(1, 2) for t in (q, k, v))
    s = (qh * scale) @ kh.transpose(-1, -2)
    j = torch.arange(Tk)
    vis = j[None, None, :] < torch.as_tensor(counts)[:, None, None]
    if causal:
        vis = vis & (j[None, None, :] <= torch.arange(Sq)[None, :, None] + offset)
    s = s.masked_fill(~vis[:, None], float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Sq, 768)


@pytest.mark.parametrize("case", [
    dict(B=6, Sq=1, Tk=29999, counts=[29999, 1, 63, 64, 65, 14003], causal=0, offset=0),
    dict(B=1, Sq=4, Tk=5000, counts=[4900], causal=1, offset=4000),   # causal masking across split boundaries
    dict(B=2, Sq=2, Tk=1499, counts=[1499, 300], causal=1, offset=255),  # ... ending exactly at one
    dict(B=4, Sq=1, Tk=200, counts=[1, 63, 64, 65], causal=0, offset=0),
    dict(B=2, Sq=450, Tk=450, counts=[450, 450], causal=1, offset=0),
    dict(B=3, Sq=37, Tk=70, counts=[70, 65, 63], causal=1, offset=33),
    dict(B=3, Sq=24, Tk=149, counts=[149, 97, 1], causal=0, offset=0),
    dict(B=1, Sq=3, Tk=1499, counts=[1499], causal=0, offset=0),
    # the language model's shapes (csrc/lm_api.hip: causal self-attention, Sq = Tk = S, counts = the rows' lengths)
    dict(B=1, Sq=300, Tk=300, counts=[300], causal=1, offset=0),       # two key splits
    dict(B=1, Sq=341, Tk=341, counts=[200], causal=1, offset=0),       # the longest S with two splits; queries past the count see its keys
    dict(B=1, Sq=1024, Tk=1024, counts=[1024], causal=1, offset=0),    # n_positions: 16 key tiles, one split
    dict(B=3, Sq=1024, Tk=1024, counts=[1024, 700, 1], causal=1, offset=0),
])
def test_op_decoder_attention(gu, case):
    B, Sq, Tk = case["B"], case["Sq"], case["Tk"]
    hu = gu.la.synth.hashed_uniform
    q = torch.from_numpy(hu(f"da/q/{B}/{Sq}", (B, Sq, 768), 5) * np.float32(2.0))
    k = torch.from_numpy(hu(f"da/k/{B}/{Tk}", (B, Tk, 768), 5) * np.float32(2.0))
    v = torch.from_numpy(hu(f"da/v/{B}/{Tk}", (B, Tk, 768), 5))
    ref = _attn_ref(q, k, v, case["counts"], case["causal"], case["offset"], 0.125)
    lib = gu.lib()
    nb = int(lib.loco_decoder_attention_scratch_bytes(B, Sq, Tk))
    scratch = torch.empty(max(nb, 4), dtype=torch.uint8, device="cuda")
    out = torch.full((B, Sq, 768), float("nan"), device="cuda")
    cnt = gu.dev(np.asarray(case["counts"]), torch.int32)
    qd, kd, vd = gu.dev(q), gu.dev(k), gu.dev(v)
    args = (gu.ptr(qd), gu.ptr(kd), gu.ptr(vd), gu.ptr(cnt), gu.ptr(out), B, Sq, Tk, case["causal"], case["offset"], 0.125, gu.ptr(scratch),
            scratch.numel(), gu.stream())
    gu.check(lib.loco_op_decoder_attention(*args), "decoder_attention")
    torch.cuda.synchronize()
    first = out.clone()
    r = gu.rel_l2(out, ref)
    record_figure("op_decoder_attention", **{k_: v_ for k_, v_ in case.items() if k_ != "counts"}, split_bytes=nb, rel_l2=r, bar=BAR_ATTN)
    assert r <= BAR_ATTN, r
    gu.check(lib.loco_op_decoder_attention(*args), "decoder_attention")
    torch.cuda.synchronize()
    assert torch.equal(first, out)  # fixed-order combine
    if Tk == 29999:
        assert nb > 0  # a long key range is split over workgroups


# ---- 6. one step under graph capture ---------------------------------------------------------------------------------------
def test_step_graph_capture(gu):
    model = full_model(gu)
    enc = model.speecht5.encoder
    lib = gu.lib()
    x, m = gu.la.synth.batch([16000, 9600])
    eo = enc(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32))
    enc_out, frames = eo.last_hidden_state, enc.last_frames
    B, T, S = 2, enc_out.shape[1], 16
    need = int(lib.loco_decoder_workspace_bytes(enc._handle, B, T, S))

    def run(graph_step):
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        logits = torch.zeros((B, 81), device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st = C.c_void_p(side.cuda_stream)
            gu.check(lib.loco_decoder_begin(enc._handle, gu.ptr(enc_out), gu.ptr(frames), B, T, S, gu.ptr(ws), need, st))
            for t in range(3):
                gu.check(lib.loco_decoder_step(enc._handle, B, T, S, t, gu.ptr(logits), gu.ptr(ws), need, st))
            side.synchronize()
            if graph_step:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    gu.check(lib.loco_decoder_step(enc._handle, B, T, S, 3, gu.ptr(logits), gu.ptr(ws), need, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                g.replay()
                g.replay()  # a step only reads what earlier steps wrote: replaying it changes nothing
            else:
                gu.check(lib.loco_decoder_step(enc._handle, B, T, S, 3, gu.ptr(logits), gu.ptr(ws), need, st))
            toks = torch.zeros((B, S), dtype=torch.int32, device="cuda")
            gu.check(lib.loco_decoder_read_tokens(enc._handle, B, T, S, gu.ptr(toks), None, gu.ptr(ws), need, st))
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
        return logits.cpu(), toks.cpu()

    l0, t0 = run(False)
    l1, t1 = run(True)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    assert bool((t0[:, 0] == 2).all()) and bool(torch.isfinite(l0).all())


# ---- 7. the C ABI's own answers on real handles ------------------------------------------------------------------------------
def raw_handle(gu, layers, weights):
    """A handle built through the C ABI alone (no Python module): loco_create + loco_set_weight per tensor; the caller finalizes."""
    lib = gu.lib()
    cfg = gu._libmod.LocoConfig()
    lib.loco_default_config(C.byref(cfg))
    cfg.layers = layers
    h = C.c_void_p(lib.loco_create(C.byref(cfg)))
    assert h.value
    for k, v in weights.items():
        t = gu.dev(np.ascontiguousarray(v))
        gu.check(lib.loco_set_weight(h, k.encode(), gu.ptr(t), (C.c_int64 * t.dim())(*t.shape), t.dim()), k)
    return h


def test_cabi_workspace_and_error_codes(gu):
    model = full_model(gu)
    enc = model.speecht5.encoder
    lib = gu.lib()
    x, m = gu.la.synth.batch([16000, 9600])
    eo = enc(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32))
    enc_out, frames = eo.last_hidden_state, enc.last_frames
    h, B, T = enc._handle, 2, enc_out.shape[1]
    assert lib.loco_has_decoder(h) == 1
    wb = lambda b, t, s: int(lib.loco_decoder_workspace_bytes(h, b, t, s))  # noqa: E731
    base = wb(2, 49, 40)
    assert base > 0
    for b, t, s in ((3, 49, 40), (2, 50, 40), (2, 49, 41), (64, 49, 40), (2, 29999, 40), (2, 49, 450)):
        assert wb(b, t, s) >= base, (b, t, s)
    assert wb(1, 49, 40) <= base and wb(2, 1, 40) <= base and wb(2, 49, 2) <= base
    assert [wb(2, 49, s) for s in range(2, 451, 64)] == sorted(wb(2, 49, s) for s in range(2, 451, 64))
    assert [wb(2, t, 40) for t in (1, 249, 256, 257, 1499, 29999)] == sorted(wb(2, t, 40) for t in (1, 249, 256, 257, 1499, 29999))
    assert [wb(b, 249, 40) for b in (1, 2, 7, 33, 64)] == sorted(wb(b, 249, 40) for b in (1, 2, 7, 33, 64))
    need = wb(B, T, 450)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st = gu.stream()
    # positions beyond max_text_positions: LOCO_E_INVALID naming the limit, from every entry point
    assert lib.loco_decoder_begin(h, gu.ptr(enc_out), gu.ptr(frames), B, T, 451, gu.ptr(ws), need, st) == -1
    assert b"450" in lib.loco_last_error()
    ids = torch.full((B, 451), 5, dtype=torch.int32, device="cuda")
    logits = torch.zeros((B, 451, 81), device="cuda")
    assert lib.loco_decoder_forward(h, gu.ptr(enc_out), gu.ptr(frames), B, T, gu.ptr(ids), 451, gu.ptr(logits), None, gu.ptr(ws), need, st) == -1
    assert b"450" in lib.loco_last_error()
    toks = torch.zeros((B, 451), dtype=torch.int32)
    assert lib.loco_decoder_generate(h, gu.ptr(enc_out), gu.ptr(frames), B, T, 451, C.c_void_p(toks.data_ptr()), None, None, None, gu.ptr(ws), need, st) == -1
    assert b"450" in lib.loco_last_error()
    assert lib.loco_decoder_begin(h, gu.ptr(enc_out), gu.ptr(frames), B, T, 450, gu.ptr(ws), need, st) == 0  # the limit itself is fine
    # a workspace one byte short: LOCO_E_WORKSPACE
    assert lib.loco_decoder_begin(h, gu.ptr(enc_out), gu.ptr(frames), B, T, 450, gu.ptr(ws), need - 1, st) == -3
    assert lib.loco_decoder_step(h, B, T, 450, 0, None, gu.ptr(ws), need - 1, st) == -3
    assert lib.loco_decoder_forward(h, gu.ptr(enc_out), gu.ptr(frames), B, T, gu.ptr(ids), 450, gu.ptr(logits), None, gu.ptr(ws), wb(B, T, 450) - 1, st) == -3
    # a step that would write past the token buffer, more clips than the step takes
    assert lib.loco_decoder_step(h, B, T, 450, 449, None, gu.ptr(ws), need, st) == -1
    assert lib.loco_decoder_begin(h, gu.ptr(enc_out), gu.ptr(frames), 65, T, 4, gu.ptr(ws), need, st) in (-1, -3)
    torch.cuda.synchronize()
    # an encoder-only handle: LOCO_E_STATE, no decoder, no workspace to size
    eo_model, _ = gu.model(layers=1)
    e1 = eo_model.speecht5.encoder
    y = e1(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32)).last_hidden_state
    assert lib.loco_has_decoder(e1._handle) == 0 and lib.loco_decoder_workspace_bytes(e1._handle, 2, 49, 40) == 0
    assert lib.loco_decoder_begin(e1._handle, gu.ptr(y), None, 2, y.shape[1], 40, gu.ptr(ws), need, st) == -2
    assert b"decoder" in lib.loco_last_error()
    assert lib.loco_decoder_forward(e1._handle, gu.ptr(y), None, 2, y.shape[1], gu.ptr(ids), 40, gu.ptr(logits), None, gu.ptr(ws), need, st) == -2


def test_cabi_partial_decoder_names_what_is_missing(gu):
    lib = gu.lib()
    synth = gu.la.synth
    dec = synth.decoder_state_dict(0, layers=2)
    enc_w = {k: v for k, v in synth.encoder_state_dict(0, 1).items()}
    buf = C.create_string_buffer(1 << 16)
    h = raw_handle(gu, 1, enc_w)
    try:
        assert lib.loco_missing_weights(h, buf, len(buf)) == 0 and lib.loco_has_decoder(h) == 0  # no decoder key: the answer it always gave
        part = {k: v for k, v in dec.items() if k.startswith("decoder.wrapped_decoder.layers.1.self_attn.")}  # 8 tensors of layer 1 only
        t = {k: gu.dev(v) for k, v in part.items()}
        for k, v in t.items():
            gu.check(lib.loco_set_weight(h, k.encode(), gu.ptr(v), (C.c_int64 * v.dim())(*v.shape), v.dim()), k)
        n = lib.loco_missing_weights(h, buf, len(buf))
        names = buf.value.decode().split(",")
        per_layer = 8 * 2 + 3 * 2 + 4
        assert n == len(names) == 1 + 2 * per_layer - 8  # the tied embedding once, layer 0 whole, the rest of layer 1
        assert "decoder.prenet.embed_tokens.weight" in names and "text_decoder_postnet.lm_head.weight" not in names
        assert "decoder.wrapped_decoder.layers.0.encoder_attn.v_proj.bias" in names
        assert "decoder.wrapped_decoder.layers.1.final_layer_norm.weight" in names
        assert not any(k in names for k in part)
        assert lib.loco_has_decoder(h) == 0 and lib.loco_decoder_workspace_bytes(h, 2, 49, 40) == 0
        assert lib.loco_finalize_weights(h, gu.stream()) == -2 and b"decoder.prenet.embed_tokens.weight" in lib.loco_last_error()
        # a wrong shape and an unknown decoder key are refused by name
        bad = gu.dev(np.zeros((4, 4), np.float32))
        assert lib.loco_set_weight(h, b"decoder.wrapped_decoder.layers.0.self_attn.q_proj.weight", gu.ptr(bad), (C.c_int64 * 2)(4, 4), 2) == -1
        assert b"size mismatch" in lib.loco_last_error()
        assert lib.loco_set_weight(h, b"decoder.wrapped_decoder.layer_norm.weight", gu.ptr(bad), (C.c_int64 * 2)(4, 4), 2) == -1
        # the rest, lm_head standing in for the tied pair: complete
        rest = {k: gu.dev(v) for k, v in dec.items() if k not in part and k != "decoder.prenet.embed_tokens.weight"}
        for k, v in rest.items():
            gu.check(lib.loco_set_weight(h, k.encode(), gu.ptr(v), (C.c_int64 * v.dim())(*v.shape), v.dim()), k)
        assert lib.loco_missing_weights(h, buf, len(buf)) == 0 and lib.loco_has_decoder(h) == 1
        gu.check(lib.loco_finalize_weights(h, gu.stream()), "finalize")
        assert lib.loco_decoder_workspace_bytes(h, 2, 49, 40) > 0
    finally:
        lib.loco_destroy(h)


def test_cabi_generated_position_table(gu, g13):
    """A C caller that does not hand over HF's position buffer gets the library's own table (finalize_decoder): golden B through a
    handle built by the raw ABI, against HF and against the Python path (which uploads torch's table)."""
    lib = gu.lib()
    synth = gu.la.synth
    w = dict(synth.encoder_state_dict(0, 1))
    w.update(synth.decoder_state_dict(int(g13["decoder_seed"])))
    h = raw_handle(gu, 1, w)
    try:
        gu.check(lib.loco_finalize_weights(h, gu.stream()), "finalize")
        enc_out = gu.dev((synth.hashed_uniform("g13/enc", (3, 149, 768), 0) * np.float32(1.5)).astype(np.float32))
        ids = gu.dev(g13["b_ids"], torch.int32)
        frames = gu.dev(np.asarray([149, 97, 1]), torch.int32)
        need = int(lib.loco_decoder_workspace_bytes(h, 3, 149, 24))
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        logits = torch.zeros((3, 24, 81), device="cuda")
        gu.check(lib.loco_decoder_forward(h, gu.ptr(enc_out), gu.ptr(frames), 3, 149, gu.ptr(ids), 24, gu.ptr(logits), None, gu.ptr(ws), need,
                                          gu.stream()), "loco_decoder_forward")
        torch.cuda.synchronize()
        py, _ = decoder_forward(gu, full_model(gu), enc_out, frames, ids, hidden=False)
        torch.cuda.synchronize()
        r_hf, r_py = gu.rel_l2(logits, g13["b_logits32"]), gu.rel_l2(logits, py)
        record_figure("decoder_generated_position_table", vs_hf32=r_hf, vs_python_path=r_py)
        print("generated table: vs HF", r_hf, "vs python path", r_py)
        assert r_hf <= BAR and r_py <= BAR
    finally:
        lib.loco_destroy(h)
