"""output_attentions=True on the GPU: the attention_probs kernel (loco-asr_amd/csrc/attention_probs.hip) through the speech and text
encoders and as a standalone op, against HF's float64 probabilities (g12) and fp64 torch restatements.

Bars: max |dP| <= 1e-5 in precision modes f32 and f16x3 (the issue's 2e-5, tightened to 4x the measured figure), 5e-3 in f16x2; masked keys exactly 0; row sums within 1e-5 of 1.
Every measured figure goes to record_figure.  The kernel's own contract -- per element, on poisoned inputs, chained behind a real attention
launch -- is tests/test_gpu_attention_probs_contract.py; here one forward on a 0xFF-filled workspace guards the same hazard at model level."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden, record_figure

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpu_util import check, la, lib, model, ptr, stream

# measured on MI355X (profiles/attn_probs_parity.jsonl): at most 2.5e-6 in f32 / f16x3 (g12, restatements, op level), 1.7e-3 in f16x2
TOL = {"f32": 1e-5, "f16x3": 1e-5, "f16x2": 5e-3}
LOCO_E_INVALID, LOCO_E_STATE = -1, -2
_text_cache = {}


def text_model(layers=12, precision="f16x3", mod=None):
    key = (layers, mod is not None)
    if key not in _text_cache or mod is not None:
        sd = la.synth.encoder_state_dict(0, layers)
        if mod is not None:
            mod(sd)
        _, enc = la.synth.split_state_dict(sd)
        tsd = la.synth.text_prenet_state_dict(0)
        pre = {k[len("text_prenet."):]: torch.from_numpy(np.asarray(v)) for k, v in tsd.items()}
        pre["encode_positions.pe"] = la.scaled_positional_table(450)[None]
        m = la.SpeechT5ForTextToSpeechMI355X.from_state_dicts(pre, {k: torch.from_numpy(v) for k, v in enc.items()}, layers=layers)
        full = dict(sd)
        full.update(tsd)
        _text_cache[key] = (m.to("cuda"), full)
    m, sd = _text_cache[key]
    m.speecht5.encoder.precision = precision
    return m, sd


def speech_call(enc, lengths, **kw):
    x, m = la.synth.batch(lengths)
    out = enc(input_values=torch.from_numpy(x).cuda(), attention_mask=torch.from_numpy(m).cuda(), **kw)
    torch.cuda.synchronize()
    return out


def frames_of(lengths):
    return [int(lib().loco_output_frames(n)) for n in lengths]


def check_structure(P, frames, what):
    """masked keys exactly 0, row sums within 1e-5 of 1, no NaN; -> max |row sum - 1|"""
    assert torch.isfinite(P).all(), what
    worst = 0.0
    for b, f in enumerate(frames):
        assert (P[b, ..., f:] == 0).all(), f"{what}: clip {b} has non-zero probability on a masked key"
        worst = max(worst, float((P[b].double().sum(-1) - 1).abs().max()))
    assert worst <= 1e-5, (what, worst)
    return worst


# ---- 1. g12: HF float64, speech and text ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32", "f16x2"])
def test_g12_speech_against_hf(precision):
    g = golden("g12_attentions.npz")
    m, _ = model(precision=precision)
    enc = m.speecht5.encoder
    a1 = speech_call(enc, [int(v) for v in g["g1_lengths"]], output_attentions=True).attentions
    assert len(a1) == 12
    d1 = max(float((a1[l].cpu().double() - torch.from_numpy(g["g1_probs"][i]).double()).abs().max())
             for i, l in enumerate(g["g1_layers"]))
    lengths = [int(v) for v in g["g2_lengths"]]
    a2 = speech_call(enc, lengths, output_attentions=True).attentions
    fr = frames_of(lengths)
    d2, rs = 0.0, 0.0
    for l in range(12):
        P = a2[l]
        rs = max(rs, check_structure(P, fr, f"g2 layer {l}"))
        d2 = max(d2, float((P[0][:, g["g2_long_rows_index"]].cpu().double() - torch.from_numpy(g["g2_long_rows"][l]).double()).abs().max()))
        d2 = max(d2, float((P[1][:, g["g2_short_rows_index"]].cpu().double() - torch.from_numpy(g["g2_short_rows"][l]).double()).abs().max()))
    record_figure(f"attentions g12 speech {precision}", g1_max_abs=d1, g2_max_abs=d2, g2_row_sum_dev=rs, bar=TOL[precision])
    assert d1 <= TOL[precision] and d2 <= TOL[precision], (d1, d2)


@pytest.mark.parametrize("precision", ["f16x3", "f32", "f16x2"])
def test_g12_text_against_hf(precision):
    g = golden("g12_attentions.npz")
    m, _ = text_model(precision=precision)
    lengths = [int(v) for v in g["text_lengths"]]
    ids, mask = la.synth.token_ids(3, 57, lengths=lengths)
    att = m.speecht5.encoder(torch.from_numpy(ids).cuda(), attention_mask=torch.from_numpy(mask).cuda(), output_attentions=True).attentions
    torch.cuda.synchronize()
    d, rs = 0.0, 0.0
    for l in range(12):
        rs = max(rs, check_structure(att[l], lengths, f"text layer {l}"))
    for i, l in enumerate(g["text_layers"]):
        got = att[l][:, :, g["text_rows_index"]].cpu().double()
        d = max(d, float((got - torch.from_numpy(g["text_rows"][i]).double()).abs().max()))
    record_figure(f"attentions g12 text {precision}", max_abs=d, row_sum_dev=rs, bar=TOL[precision])
    assert d <= TOL[precision], d


# ---- 2. fp64 restatement from the call's own hidden states at real sizes -----------------------------------------------------
def restate(h, sd, l, frames, prefix="wrapped_encoder."):
    """P of layer l in fp64 from its input hidden state h [B,T,768] (HF modeling_speecht5.py:891-955)."""
    d = lambda k: torch.from_numpy(np.asarray(sd[prefix + k])).cuda().double()  # noqa: E731
    a = f"layers.{l}.attention."
    h = h.double()
    B, T, _ = h.shape
    q = ((h @ d(a + "q_proj.weight").T + d(a + "q_proj.bias")) * 0.125).view(B, T, 12, 64).transpose(1, 2)
    k = (h @ d(a + "k_proj.weight").T + d(a + "k_proj.bias")).view(B, T, 12, 64).transpose(1, 2)
    pe = d("embed_positions.pe_k.weight")  # [320, 64]
    ar = torch.arange(T, device="cuda")
    idx = ((ar[:, None] - ar[None, :]).clamp(-160, 159) + 160)
    S = q @ k.transpose(-1, -2) + torch.gather(q @ pe.T, -1, idx.expand(B, 12, T, T))
    for b, f in enumerate(frames):
        S[b, ..., f:] = -torch.inf
    return torch.softmax(S, -1)


@pytest.mark.parametrize("lengths", [[480000, 276800], [40000, 33000, 20000]], ids=["30s+17.3s", "B3_T124"])
@pytest.mark.parametrize("precision", ["f16x3", "f32", "f16x2"])
def test_restatement_at_real_sizes(lengths, precision):
    m, sd = model(precision=precision)
    out = speech_call(m.speecht5.encoder, lengths, output_attentions=True, output_hidden_states=True)
    fr = frames_of(lengths)
    T = out.last_hidden_state.shape[1]
    assert lengths[0] != 40000 or T % 32 != 0
    worst, rs = 0.0, 0.0
    for l in range(12):
        ref = restate(out.hidden_states[l], sd, l, fr)
        P = out.attentions[l]
        rs = max(rs, check_structure(P, fr, f"layer {l}"))
        worst = max(worst, float((P.double() - ref).abs().max()))
        del ref
    record_figure(f"attentions restatement {precision} {lengths}", T=T, max_abs=worst, row_sum_dev=rs, bar=TOL[precision])
    assert worst <= TOL[precision], worst


def test_poisoned_workspace_reaches_no_attention():
    """The f16x3 forward hands the probabilities kernel the table scratch its attention launch has just filled, inside a torch.empty
    workspace.  With T >= 225 and a clip of at most 64 frames that launch forms no table block for the padded queries from row 224 on;
    the probabilities kernel must read nothing there.  The workspace is filled with 0xFF bytes (fp32 NaN) between two calls.  A
    regression guard only -- other stages of the forward may overwrite the region first; the proof is the x3_chain form of
    tests/test_gpu_attention_probs_contract.py."""
    m, sd = model(layers=2, precision="f16x3")
    enc = m.speecht5.encoder
    lengths = [80000, 4800]
    speech_call(enc, lengths, output_attentions=True)  # sizes the workspace
    enc._workspace.fill_(0xFF)
    out = speech_call(enc, lengths, output_attentions=True, output_hidden_states=True)
    fr = frames_of(lengths)
    T = out.last_hidden_state.shape[1]
    assert T >= 225 and min(fr) <= 64 and len(out.attentions) == 2
    worst = 0.0
    for l in range(2):
        P = out.attentions[l]
        rs = check_structure(P, fr, f"poisoned workspace, layer {l}")
        worst = max(worst, float((P.double() - restate(out.hidden_states[l], sd, l, fr)).abs().max()))
    record_figure("attentions poisoned workspace f16x3", T=T, frames=fr, max_abs=worst, row_sum_dev=rs, bar=TOL["f16x3"])
    assert worst <= TOL["f16x3"], worst


# ---- 3. op level ----------------------------------------------------------------------------------------------------------
def op_inputs(B, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, T, 2304, generator=g)
    qkv[..., :768] *= 0.125
    qp = torch.randn(B, 12, T, 320, generator=g) * 0.5
    return qkv.cuda(), qp.cuda()


def op_reference(qkv, qp, frames):
    B, T, _ = qkv.shape
    q = qkv[..., :768].double().view(B, T, 12, 64).transpose(1, 2)
    k = qkv[..., 768:1536].double().view(B, T, 12, 64).transpose(1, 2)
    ar = torch.arange(T, device="cuda")
    idx = ((ar[:, None] - ar[None, :]).clamp(-160, 159) + 160)
    S = q @ k.transpose(-1, -2) + torch.gather(qp.double(), -1, idx.expand(B, 12, T, T))
    for b, f in enumerate(frames):
        S[b, ..., f:] = -torch.inf
    return torch.softmax(S, -1)


def split(x):
    hi = x.half()
    return hi.contiguous(), (x - hi.float()).half().contiguous()


def run_op(form, qkv, qp, frames, terms=3):
    B, T, _ = qkv.shape
    P = torch.full((B, 12, T, T), float("nan"), device="cuda")
    fr = torch.tensor(frames, dtype=torch.int32, device="cuda")
    if form == "f32":
        check(lib().loco_op_attention_probs(ptr(qkv), ptr(qp), ptr(fr), ptr(P), B, T, stream()))
    else:
        qh, ql = split(qkv[..., :768].reshape(B * T, 768).contiguous())
        kh, kl = split(qkv[..., 768:1536].reshape(B * T, 768).contiguous())
        check(lib().loco_op_attention_probs_f16x3(ptr(qh), ptr(ql), ptr(kh), ptr(kl), ptr(qp), ptr(fr), ptr(P), B, T, terms, stream()))
    torch.cuda.synchronize()
    return P


def stale_outside_read_columns(qp, frames):
    """NaN in every qp entry no valid key reads: what a masked key would find in the f16x3 launch's scratch.  A host-side model, and a
    generous one: the real scratch also lacks the whole rows of padded queries whose every key is past-clipped
    (tests/test_gpu_attention_probs_contract.py chains a real launch and poisons those too)."""
    B, _, T, _ = qp.shape
    qp = qp.clone()
    i = torch.arange(T, device="cuda")[:, None]
    c = torch.arange(320, device="cuda")[None, :]
    for b, f in enumerate(frames):
        lo = (i - f + 1).clamp(-160, 159) + 160
        hi = i.clamp(-160, 159) + 160
        qp[b][:, ((c < lo) | (c > hi))] = float("nan")
    return qp


@pytest.mark.parametrize("T", [1, 31, 33, 64, 65, 257, 1499])
@pytest.mark.parametrize("form", ["f32", "f16x3"])
def test_op_against_fp64(T, form):
    worst = 0.0
    for fv in sorted({1, max(1, T // 2), T}):
        frames = [fv, T]
        qkv, qp = op_inputs(2, T, seed=T + fv)
        ref = op_reference(qkv, qp, frames)
        if form == "f16x3":
            qp = stale_outside_read_columns(qp, frames)
        P = run_op(form, qkv, qp, frames)
        check_structure(P, frames, f"T={T} frames={fv}")
        if fv == 1:
            assert (P[0, ..., 0] == 1.0).all()
        worst = max(worst, float((P.double() - ref).abs().max()))
    record_figure(f"attention_probs op {form} T={T}", max_abs=worst)
    assert worst <= TOL["f32"], worst


def test_op_two_terms_and_null_frames():
    qkv, qp = op_inputs(1, 100, seed=3)
    ref = op_reference(qkv, qp, [100])
    P2 = run_op("f16x3", qkv, qp, [100], terms=2)
    d2 = float((P2.double() - ref).abs().max())
    P = torch.empty(1, 12, 100, 100, device="cuda")
    check(lib().loco_op_attention_probs(ptr(qkv), ptr(qp), None, ptr(P), 1, 100, stream()))
    torch.cuda.synchronize()
    d0 = float((P.double() - ref).abs().max())
    record_figure("attention_probs op terms=2 / frames NULL", terms2_max_abs=d2, null_frames_max_abs=d0)
    assert d2 <= 5e-3 and d0 <= TOL["f32"]
    assert lib().loco_op_attention_probs_f16x3(ptr(qkv), ptr(qkv), ptr(qkv), ptr(qkv), ptr(qp), None, ptr(P), 1, 100, 4, stream()) == LOCO_E_INVALID


@pytest.mark.parametrize("form", ["f32", "f16x3"])
def test_op_outlier_key_gives_no_nan(form):
    T, i, js = 64, 40, 20
    qkv, qp = op_inputs(1, T, seed=5)
    qp[0, :, i, (i - js) + 160] += 80.0  # key js scores 80 above the rest in row i (|i - js| < 159: a column of its own)
    P = run_op(form, qkv, qp, [T])
    assert torch.isfinite(P).all()
    ref = op_reference(qkv, qp, [T])
    assert float((P.double() - ref).abs().max()) <= TOL["f32"]
    assert (P[0, :, i, js] > 0.999).all()


def test_op_more_than_2_31_elements():
    """B = 1, T = 13 400: 2.15e9 elements in one layer's P; frames < T.  Sampled rows, including the last one."""
    T, f = 13400, 12001
    qkv, qp = op_inputs(1, T, seed=9)
    P = torch.full((1, 12, T, T), float("nan"), device="cuda")
    assert P.numel() > 2 ** 31
    fr = torch.tensor([f], dtype=torch.int32, device="cuda")
    qh, ql = split(qkv[..., :768].reshape(T, 768).contiguous())
    kh, kl = split(qkv[..., 768:1536].reshape(T, 768).contiguous())
    check(lib().loco_op_attention_probs_f16x3(ptr(qh), ptr(ql), ptr(kh), ptr(kl), ptr(qp), ptr(fr), ptr(P), 1, T, 3, stream()))
    torch.cuda.synchronize()
    rows = torch.tensor([0, 1, 6700, f - 1, f, T - 1], device="cuda")
    q = qkv[0, :, :768].double().view(T, 12, 64).transpose(0, 1)[:, rows]          # [12, R, 64]
    k = qkv[0, :, 768:1536].double().view(T, 12, 64).transpose(0, 1)              # [12, T, 64]
    idx = ((rows[:, None] - torch.arange(T, device="cuda")[None, :]).clamp(-160, 159) + 160)
    S = q @ k.transpose(-1, -2) + torch.gather(qp[0][:, rows].double(), -1, idx.expand(12, -1, -1))
    S[..., f:] = -torch.inf
    ref = torch.softmax(S, -1)
    got = P[0][:, rows].double()
    d = float((got - ref).abs().max())
    record_figure("attention_probs op T=13400", max_abs=d)
    assert torch.isfinite(got).all() and (got[..., f:] == 0).all()
    assert d <= TOL["f32"], d
    assert not torch.isnan(P[0, 11, T - 1, T - 1]) and not torch.isnan(P[0, 11, T - 1, 0])


# ---- 4. the default path is unchanged ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32", "f16x2"])
def test_default_outputs_bitwise_unchanged(precision):
    m, _ = model(precision=precision)
    enc = m.speecht5.encoder
    enc.streams = 1
    try:
        lengths = [80000, 48000]
        a = speech_call(enc, lengths, output_hidden_states=True)
        b = speech_call(enc, lengths, output_hidden_states=True, output_attentions=True)
        c = speech_call(enc, lengths)
        assert torch.equal(a.last_hidden_state, b.last_hidden_state) and torch.equal(a.last_hidden_state, c.last_hidden_state)
        assert all(torch.equal(x, y) for x, y in zip(a.hidden_states, b.hidden_states))
    finally:
        enc.streams = 2
    t, _ = text_model(precision=precision)
    ids, mask = la.synth.token_ids(3, 57, lengths=[57, 31, 44])
    ids, mask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    x = t.speecht5.encoder(ids, attention_mask=mask, output_hidden_states=True)
    y = t.speecht5.encoder(ids, attention_mask=mask, output_hidden_states=True, output_attentions=True)
    assert torch.equal(x.last_hidden_state, y.last_hidden_state)
    assert all(torch.equal(u, v) for u, v in zip(x.hidden_states, y.hidden_states))


# ---- 5. range fallback ------------------------------------------------------------------------------------------------------
FFN1 = "wrapped_encoder.layers.0.feed_forward.intermediate_dense."


def overflow(sd):
    for k in ("weight", "bias"):
        sd[FFN1 + k] = (sd[FFN1 + k] * np.float32(40000.0)).astype(np.float32)


def test_range_fallback_rewrites_attentions():
    sd = la.synth.encoder_state_dict(0, 2)
    overflow(sd)
    pre, encsd = la.synth.split_state_dict(sd)
    m = la.SpeechT5ForSpeechToTextMI355X(2)
    m.speecht5.encoder.wrapped_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in encsd.items()})
    m.speecht5.encoder.prenet.load_state_dict({k: torch.from_numpy(v) for k, v in pre.items()})
    enc = m.to("cuda").speecht5.encoder
    lengths = [24000, 16000, 9000]
    a = speech_call(enc, lengths, output_attentions=True)
    assert enc.last_range_fallback
    enc.precision = "f32"
    b = speech_call(enc, lengths, output_attentions=True)
    assert all(torch.equal(x, y) for x, y in zip(a.attentions, b.attentions))

    t, _ = text_model(layers=2, mod=overflow)
    ids, mask = la.synth.token_ids(3, 57, lengths=[57, 31, 44])
    ids, mask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    x = t.speecht5.encoder(ids, attention_mask=mask, output_attentions=True)
    assert t.speecht5.encoder.last_range_fallback
    t.speecht5.encoder.precision = "f32"
    y = t.speecht5.encoder(ids, attention_mask=mask, output_attentions=True)
    assert all(torch.equal(u, v) for u, v in zip(x.attentions, y.attentions))
    assert all(torch.isfinite(u).all() for u in x.attentions)


# ---- 6. contract and errors ----------------------------------------------------------------------------------------------
def test_contract_shapes_and_tuple_order():
    m, _ = model()
    enc = m.speecht5.encoder
    lengths = [16000, 9600]
    o = speech_call(enc, lengths, output_attentions=True)
    T = o.last_hidden_state.shape[1]
    assert o.hidden_states is None and len(o.attentions) == 12
    for P in o.attentions:
        assert P.shape == (2, 12, T, T) and P.dtype == torch.float32 and P.device == o.last_hidden_state.device
    t1 = speech_call(enc, lengths, output_attentions=True, output_hidden_states=True, return_dict=False)
    assert len(t1) == 3 and len(t1[1]) == 13 and len(t1[2]) == 12 and t1[2][0].shape == (2, 12, T, T)
    t2 = speech_call(enc, lengths, output_attentions=True, return_dict=False)
    assert len(t2) == 2 and len(t2[1]) == 12 and t2[1][0].dim() == 4
    assert all(torch.equal(x, y) for x, y in zip(t1[2], o.attentions))
    z, _ = model(layers=0)
    assert speech_call(z.speecht5.encoder, lengths, output_attentions=True).attentions == ()
    zt, _ = text_model(layers=0)
    ids, _ = la.synth.token_ids(2, 9)
    assert zt.speecht5.encoder(torch.from_numpy(ids).cuda(), output_attentions=True).attentions == ()


def test_bound_outputs_refuse_async_and_packed_forwards():
    m, _ = model()
    enc = m.speecht5.encoder
    speech_call(enc, [16000])  # handle exists
    L = lib()
    h = enc._handle
    buf = [torch.empty(1, device="cuda") for _ in range(12)]
    ptrs = (C.c_void_p * 12)(*[b.data_ptr() for b in buf])
    assert L.loco_set_attention_outputs(h, ptrs, 11) == LOCO_E_INVALID
    check(L.loco_set_attention_outputs(h, ptrs, 12))
    try:
        st = torch.empty(int(L.loco_status_bytes()), dtype=torch.uint8).pin_memory()
        d = ptr(buf[0])
        pad = (C.c_int64 * 1)(16000)
        assert L.loco_forward_async(h, -1, d, None, 1, 16000, d, d, None, d, 1 << 30, stream(), ptr(st)) == LOCO_E_STATE
        assert L.loco_forward_packed(h, -1, d, None, None, 1, 16000, pad, d, d, None, d, 1 << 30, stream(), ptr(st)) == LOCO_E_STATE
    finally:
        check(L.loco_set_attention_outputs(h, None, 0))
    speech_call(enc, [16000])  # unbound again: the default path works
    t, _ = text_model()
    ids, _ = la.synth.token_ids(1, 8)
    ids = torch.from_numpy(ids).cuda()
    t.speecht5.encoder(ids)  # handle exists
    ht = t.speecht5.encoder._handle
    check(L.loco_set_attention_outputs(ht, ptrs, 12))
    try:
        assert L.loco_forward_text_async(ht, -1, d, None, 1, 8, d, d, None, d, 1 << 30, stream(), ptr(st)) == LOCO_E_STATE
    finally:
        check(L.loco_set_attention_outputs(ht, None, 0))
    t.speecht5.encoder(ids)


def test_profiling_bucket_counts_one_launch_per_layer():
    m, _ = model()
    enc = m.speecht5.encoder
    enc.set_profiling(True)
    try:
        enc.profile_reset()
        speech_call(enc, [16000, 9600], output_attentions=True)
        st = {s["name"]: s for s in enc.profile_read()}
        assert st["attention_probs"]["launches"] == 12
        enc.profile_reset()
        speech_call(enc, [16000, 9600])
        assert "attention_probs" not in {s["name"] for s in enc.profile_read()}
    finally:
        enc.set_profiling(False)
