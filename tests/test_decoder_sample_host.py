"""Sampling in the text decoder, everything that needs no device: the CPU restatement of the rule (tests/decoder_sample_ref.py) against
Random123's known answers and the installed transformers' logits warpers, hand-made rows for what random floats never hit, the
arguments ``sample`` / ``sample_many`` refuse, and what the new C-ABI entry points answer before any launch."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import decoder_sample_ref as ref

la = importlib.import_module("loco-asr_amd")
dec = importlib.import_module("loco-asr_amd.decoder")
_libmod = importlib.import_module("loco-asr_amd._lib")


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    f = 0xFFFFFFFF
    for counter, key, want in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                               ((f, f, f, f), (f, f), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join(f"{w:08x}" for w in ref.philox4x32_10(counter, key)) == want


def test_uniform_is_24_bits_of_word_0():
    seed = 0x299f31d0a4093822  # the third known answer's key as (low, high) words of one seed
    u = ref.uniform(seed, 0x243f6a88, 0x85a308d3, 0x13198a2e)
    assert ref.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))[0] >> 8 == int(u * 2 ** 24)
    us = [ref.uniform(7, u_, h, t) for u_ in range(3) for h in range(3) for t in range(1, 4)]
    assert all(0 <= v < 1 and float(np.float32(v)) == v for v in us) and len(set(us)) == 27
    assert ref.uniform(7, 1, 2, 3) != ref.uniform(8, 1, 2, 3)


# ---- the keep rule against HF's warpers ---------------------------------------------------------------------------------------------
def hf_keep(row, temperature, top_k, top_p):
    lp = pytest.importorskip("transformers.generation.logits_process")
    scores = (torch.as_tensor(row, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)).double()[None]
    ids = torch.zeros((1, 1), dtype=torch.long)
    if top_k:
        scores = lp.TopKLogitsWarper(top_k=int(top_k))(ids, scores)
    if top_p < 1:
        scores = lp.TopPLogitsWarper(top_p=float(top_p))(ids, scores)
    return torch.isfinite(scores[0])


def test_keep_mask_equals_hf_warpers():
    """400 seeded rows, V in 2 .. 129, random temperature / top-k / top-p (random floats carry no ties): identical masks.  A row whose
    nearest A_i lies within 1e-6 of 1 - top_p may be skipped; under 1 % are."""
    rng = np.random.default_rng(20240)
    skipped = 0
    for case in range(400):
        V = int(rng.integers(2, 130))
        row = (rng.standard_normal(V) * rng.choice([1.0, 4.0])).astype(np.float32)
        T = float(np.float32(rng.choice([0.5, 0.7, 1.0, 1.3, 8.0])))
        k = int(rng.choice([0, 0, 1, 2, 5, V // 2, V, V + 3]))
        p = float(np.float32(rng.choice([1.0, 0.95, 0.9, 0.5, 0.3, float(rng.uniform(0.05, 0.999))])))
        keep, A = ref.keep_mask(row, T, k, p)
        if p < 1 and float((A[~torch.isnan(A)] - (1 - p)).abs().min()) < 1e-6:
            skipped += 1
            continue
        assert torch.equal(keep, hf_keep(row, T, k, p)), (case, V, T, k, p)
        assert bool(keep[int(np.argmax(row))])
    assert skipped < 4, skipped


def test_handmade_rows():
    t = lambda *v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    # the tie rule: masses 1 : e : e : e^2, A = .072, .466, .466, 1 -- the equal pair is kept or dropped as a whole
    row = t(0, 1, 1, 2)
    assert ref.keep_mask(row, 1.0, 0, 0.7)[0].tolist() == [False, True, True, True]
    assert ref.keep_mask(row, 1.0, 0, 0.5)[0].tolist() == [False, False, False, True]
    # top-k: ties at the threshold all survive
    assert ref.keep_mask(t(3, 1, 3, 2, 2), 1.0, 3, 1.0)[0].tolist() == [True, False, True, True, True]
    assert ref.keep_mask(t(3, 1, 3, 2, 2), 1.0, 1, 1.0)[0].tolist() == [True, False, True, False, False]
    assert ref.keep_mask(t(3, 1, 3, 2, 2), 1.0, 2, 1.0)[0].tolist() == [True, False, True, False, False]
    # top_k >= V and top_p = 1: off
    for k in (0, 5, 9):
        assert bool(ref.keep_mask(t(3, 1, 3, 2, 2), 0.7, k, 1.0)[0].all())
    # top-p over the survivors only: of (2, 1 | 0, 0) the pair left by top-k = 2 has masses .731, .269
    assert ref.keep_mask(t(2, 1, 0, 0), 1.0, 2, 0.7)[0].tolist() == [True, False, False, False]
    assert ref.keep_mask(t(2, 1, 0, 0), 1.0, 2, 0.75)[0].tolist() == [True, True, False, False]
    # a top_p so small that no A exceeds 1 - top_p in the working precision: the argmax alone (min_tokens_to_keep = 1)
    assert ref.keep_mask(t(1, 5, 5, 2), 1.0, 0, 1e-30, dtype=torch.float32)[0].tolist() == [False, True, False, False]
    # V = 1
    assert ref.keep_mask(t(4), 2.0, 3, 0.3)[0].tolist() == [True]
    assert ref.sample_row(t(4), 2.0, 3, 0.3, 1, 0, 0, 1) == 0
    # the draw: first kept index whose prefix exceeds u Z; masses .25 .25 .5 over columns 0, 2, 3
    row, keep = t(0, 9, 0, float(np.log(2.0))), torch.tensor([True, False, True, True])
    assert [ref.draw(row, 1.0, keep, u)[0] for u in (0.0, 0.2499, 0.2501, 0.4999, 0.5001, 0.999999)] == [0, 0, 2, 2, 3, 3]
    # degenerate rows take the argmax, the first NaN winning; never an index outside the row
    nan, inf = float("nan"), float("inf")
    for row, want in ((t(nan, 1, 2), 0), (t(1, 2, nan), 2), (t(1, nan, nan), 1), (t(1, inf, 3, inf), 1), (t(-inf, -inf, -inf), 0),
                      (t(-inf, 2, -inf), 1)):
        for h in range(4):
            assert ref.sample_row(row, 0.8, 2, 0.9, 5, 3, h, 1) == want
    assert ref.degenerate(t(3e38, 0), 0.5) and not ref.degenerate(t(3e38, 0), 1.0)  # the division overflows: a +inf maximum
    assert ref.sample_row(t(1, 7, 3), 8.0, 0, 1.0, 5, 0, 0, 1, greedy=True) == 1


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_sample_argument_handling():
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=1)
    x = torch.zeros(0, 1000)
    for call in (lambda **kw: model.sample_many([], **kw), lambda **kw: model.sample(x, **kw)):
        for n in (0, 65, -1, 2.5):
            with pytest.raises(ValueError, match="num_return_sequences"):
                call(num_return_sequences=n)
        for v in (0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="temperature"):
                call(temperature=v)
        with pytest.raises(ValueError, match="top_k"):
            call(top_k=-1)
        for v in (0, 1.5, -0.1, float("nan")):
            with pytest.raises(ValueError, match="top_p"):
                call(top_p=v)
        for v in (1, 451):
            with pytest.raises(ValueError, match="max_length"):
                call(max_length=v)
        with pytest.raises(ValueError, match="slots = 65 is outside 1 .. 64"):
            call(slots=65)
        with pytest.raises(ValueError, match="seed"):
            call(seed=-1)
    with pytest.raises(ValueError, match="pack"):
        model.sample_many([], pack=0)
    with pytest.raises(ValueError, match="names 2 utterances, the batches hold 0"):
        model.sample_many([], max_length=[5, 6])
    # empty input
    hyps = model.sample_many([], num_return_sequences=3, seed=11)
    assert hyps == [] and hyps.seed == 11
    res = model.sample_many([], return_logits=True, return_scores=True, seed=12)
    assert tuple(res) == ([], [], []) and res.seed == 12 and res[0].seed == 12
    out = model.sample(x, num_return_sequences=4, seed=13, return_scores=True)
    assert isinstance(out, dec.SampleOutput) and out.sequences.shape[0] == 0 and out.seed == 13
    # seed=None: 63 bits from torch's default generator
    torch.manual_seed(5)
    a = model.sample_many([]).seed
    b = model.sample_many([]).seed
    torch.manual_seed(5)
    assert model.sample_many([]).seed == a and a != b and 0 <= a < 2 ** 63
    # generate / generate_many go on refusing the sampling keywords
    for k in ("do_sample", "temperature", "top_k", "top_p", "num_return_sequences"):
        with pytest.raises(NotImplementedError, match=k):
            model.generate_many([], **{k: 2})
    for call in (lambda m: m.sample_many([]), lambda m: m.sample(x)):
        with pytest.raises(RuntimeError, match="needs the decoder"):
            call(la.SpeechT5ForSpeechToTextMI355X(layers=1))


def test_check_sample_args_config():
    n, cfg = dec.check_sample_args(4, 0.8, 5, 0.95, 0xfedcba9876543210)
    assert n == 4 and cfg.struct_size == C.sizeof(_libmod.SampleConfig) == 24
    assert (cfg.temperature, cfg.top_k, cfg.top_p, cfg.seed) == (np.float32(0.8), 5, np.float32(0.95), 0xfedcba9876543210)
    assert dec.check_sample_args(np.int64(64), 1, torch.tensor(0), 1, 0)[0] == 64


# ---- the C ABI, before any launch -----------------------------------------------------------------------------------------------------
def test_cabi_host_only_answers():
    lib = _libmod.load()
    cfg = _libmod.SampleConfig(C.sizeof(_libmod.SampleConfig), 1.0, 0, 1.0, 0)
    for fn, args in (("loco_decoder_pool_admit_samples", (None, 4, 100, 40, 1, 2, None, None, 0, None, None, None, None, None, None, None, 0, None)),
                     ("loco_decoder_pool_step_sample", (None, 4, 100, 40, 0, 1, C.byref(cfg), None, None, None, 0, None))):
        assert getattr(lib, fn)(*args) == -1, fn  # LOCO_E_INVALID: null handle
        assert fn.encode() in lib.loco_last_error() and b"null encoder" in lib.loco_last_error()
    assert lib.loco_op_sample_tokens(None, 81, 1, 81, C.byref(cfg), None, None, None, None, None, None) == -1
    assert b"loco_op_sample_tokens" in lib.loco_last_error() and b"null" in lib.loco_last_error()


def test_cabi_sample_config_is_checked_by_field():
    """The checks that precede the launch, reached with host buffers the call never dereferences: the struct_size the library accepts
    is ctypes.sizeof of the Python struct, and every invalid field is named."""
    lib = _libmod.load()
    size = C.sizeof(_libmod.SampleConfig)
    buf = (C.c_float * 8)()
    at = C.c_void_p(C.addressof(buf))

    def answer(cfg, M=1, V=2, ld=2):
        rc = lib.loco_op_sample_tokens(at, ld, M, V, C.byref(cfg) if cfg is not None else None, at, None, at, None, None, None)
        return rc, lib.loco_last_error().decode()

    for bad_size in (size - 4, size + 8, 0):
        rc, msg = answer(_libmod.SampleConfig(bad_size, 1.0, 0, 1.0, 0))
        assert rc == -1 and "struct_size" in msg and str(size) in msg, msg
    for field, values in (("temperature", (0.0, -1.0, float("nan"), float("inf"))), ("top_k", (-1,)), ("top_p", (0.0, 1.5, -0.5, float("nan")))):
        for v in values:
            kw = dict(temperature=1.0, top_k=0, top_p=1.0)
            kw[field] = v
            rc, msg = answer(_libmod.SampleConfig(size, kw["temperature"], kw["top_k"], kw["top_p"], 0))
            assert rc == -1 and "loco_op_sample_tokens" in msg and f"loco_sample_config.{field}" in msg, (field, v, msg)
    # with the size accepted, the first complaint is about a field: sizeof(SampleConfig) is the size the library takes
    assert "temperature" in answer(_libmod.SampleConfig(size, 0.0, -1, 7.0, 0))[1]
    assert "null loco_sample_config" in answer(None)[1]
    assert "ld = 1 < V = 2" in answer(_libmod.SampleConfig(size, 1.0, 0, 1.0, 0), ld=1)[1]
    assert "must both be >= 1" in answer(_libmod.SampleConfig(size, 1.0, 0, 1.0, 0), M=0)[1]


def test_block_forms_equal_the_per_row_forms():
    """keep_mask_rows / draw_rows (what the GPU tests compare against) are keep_mask / draw row by row, ties included."""
    rng = np.random.default_rng(7)
    for V, T, k, p in ((2, 1.0, 0, 0.3), (81, 0.7, 5, 0.9), (65, 8.0, 0, 0.9), (129, 1.0, 129, 0.3), (17, 1.0, 1, 1.0), (33, 0.7, 5, 1.0)):
        rows = (rng.standard_normal((9, V)) * 4).astype(np.float32)
        rows[3] = np.round(rows[3])  # ties
        rows[4, : V // 2] = rows[4, 0]
        keep, A = ref.keep_mask_rows(rows, T, k, p)
        u = rng.uniform(0, 1, 9)
        tokens, margin, probs = ref.draw_rows(rows, T, keep, u)
        for m in range(9):
            keep1, A1 = ref.keep_mask(rows[m], T, k, p)
            assert torch.equal(keep[m], keep1), (V, m)
            assert torch.allclose(A[m], A1, rtol=0, atol=1e-14, equal_nan=True)
            token1, margin1, probs1 = ref.draw(rows[m], T, keep1, float(u[m]))
            assert int(tokens[m]) == token1 and abs(float(margin[m]) - margin1) < 1e-15 and torch.equal(probs[m], probs1)
    assert abs(ref.chi2_quantile(0.95, 10) - 18.307038) < 1e-4 and abs(ref.chi2_quantile(0.5, 2) - 2 * np.log(2)) < 1e-9


def test_transcribe_refuses_bad_sampling_arguments_before_a_model_is_built(monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    monkeypatch.setattr(tr, "build_model", lambda args: pytest.fail("a model was built"))
    base = ["--random-init", "--synthetic", "2", "--slots", "2"]
    for extra, name in ((["--nbest", "65"], "num_return_sequences"), (["--nbest", "2", "--temperature", "0"], "temperature"),
                        (["--nbest", "2", "--top-k", "-1"], "top_k"), (["--nbest", "2", "--top-p", "1.5"], "top_p"),
                        (["--nbest", "2", "--seed", "-3"], "seed")):
        with pytest.raises(SystemExit, match=name):
            tr.main(base + extra)
    with pytest.raises(SystemExit, match="--nbest needs --slots"):
        tr.main(["--random-init", "--synthetic", "2", "--nbest", "3"])
