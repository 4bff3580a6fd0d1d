"""-m gpu: the decoder slot pool (loco_decoder_pool_*, decoder.DecoderPool, generate_many) -- finished rows refilled, every slot at its
own position.  2-layer encoder and decoder weights (tests/decoder_pool_cases.py).

1. against the float64 oracle: step logits teacher-forced on the device's ids, ids against the oracle's greedy ids of each utterance
   alone under the tie rule of tests/test_gpu_decoder_oracle.py
2. neighbour independence, bitwise: pools of 2, 5 and 64 slots and the reversed order give the same ids and step logits
3. slot hygiene: a re-admitted slot and junk beyond the frame counts change no bit
4. the contract with generate; 5. limits and the C ABI's errors; 6. the CLI"""
import ctypes as C
import dataclasses
import importlib
import json

import numpy as np
import pytest
import torch

import decoder_pool_cases as pc
import decoder_sweep_cases as cases
import speecht5_decoder_oracle as dec_oracle
from conftest import record_figure
from test_gpu_decoder import BAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


_cache = {}


def small_model(gu):
    if "model" not in _cache:
        la = gu.la
        pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0, pc.ENC_LAYERS))
        _cache["dsd"] = la.synth.decoder_state_dict(pc.DEC_SEED, layers=pc.DEC_LAYERS)
        dec, post = la.synth.split_decoder_state_dict(_cache["dsd"])
        t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
        _cache["model"] = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), layers=pc.ENC_LAYERS, decoder_state_dict=t(dec),
                                                                            postnet_state_dict=t(post)).to("cuda")
    return _cache["model"]


def batches_of(gu, clips, size=2):
    return [dict(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32)) for x, m in pc.pairs(gu.la.synth, clips, size)]


def encode(gu, model, clips, caps):
    """One packed forward of the clips' pairs: (PoolItems in input order, out [B, T, 768], frames i32 [B] on the host)."""
    dec = importlib.import_module("loco-asr_amd.decoder")
    enc = model.speecht5.encoder
    ticket = enc.forward_packed_async(batches_of(gu, clips))
    ticket.result()
    out, spans = ticket.packed_output()
    frames = enc.last_frames
    items = [dec.PoolItem(key=c, enc_out=out, frames=frames, clip=c, rows=t, cap=caps[c]) for b0, nb, t in spans for c in range(b0, b0 + nb)]
    return items, out, frames.cpu()


def decode(model, items, slots, T_cap=None, poll_steps=8):
    """{key: (ids, step logits on the host)} of the items through a fresh pool."""
    dec = importlib.import_module("loco-asr_amd.decoder")
    pool = dec.DecoderPool(model.speecht5.encoder, slots, T_cap or max(it.rows for it in items), max(it.cap for it in items), torch.device("cuda", 0),
                           poll_steps=poll_steps, return_logits=True)
    pool.submit(list(items))
    return {k: (ids, lg.cpu()) for k, ids, lg in pool.drain()}


def rebased(items, out, frames=None):
    return [type(it)(key=it.key, enc_out=out, frames=it.frames if frames is None else frames, clip=it.clip, rows=it.rows, cap=it.cap) for it in items]


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) for k in a)


def consistent(ids, lg, cap):
    """What holds for every result whatever the weights: <s> first, at most cap tokens, ended by </s> or at the cap, every token the
    lowest-index argmax of its step's logits."""
    n = len(ids)
    assert ids[0] == 2 and 2 <= n <= cap and lg.shape == (n - 1, 81) and bool(torch.isfinite(lg).all())
    assert ids[1:].tolist() == lg.argmax(-1).tolist()
    assert (n == cap or ids[-1] == 2) and 2 not in ids[1:-1].tolist()


def rel_steps(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).norm(dim=-1) / b.norm(dim=-1)).max())


# ---- 1. against the float64 oracle ------------------------------------------------------------------------------------------------
def test_pool_against_oracle(gu):
    """generate_many at 3 slots, 12 utterances with their own caps: (a) step logits against the oracle teacher-forced on the device's
    ids, (b) ids against the oracle's greedy ids of each utterance alone, under the tie rule."""
    model = small_model(gu)
    clips, caps = pc.oracle_clips(gu.la.synth), pc.ORACLE_CAPS
    assert len(clips) == len(caps) == 12 and all(4800 <= n <= 48000 for _, n in clips)
    ids, logits = model.generate_many(batches_of(gu, clips), max_length=caps, slots=pc.ORACLE_SLOTS, return_logits=True)
    _, out, frames = encode(gu, model, clips, caps)  # the same packed forward: the fp32 encoder output both sides decode
    enc64 = out.cpu().double()
    dsd = _cache["dsd"]
    worst, dropped, early = 0.0, 0, 0
    for u in range(12):
        consistent(ids[u], logits[u].cpu(), caps[u])
        e, f = enc64[u:u + 1], frames[u:u + 1].long()
        tf = dec_oracle.forward(e, f, ids[u][None], dsd)[0, :-1]
        r = rel_steps(logits[u].cpu(), tf)
        worst = max(worst, r)
        ids_o, _, lengths_o, gaps = dec_oracle.greedy(e, f, dsd, caps[u])
        stop = cases.first_low_gap_step(gaps, lengths_o)[0]
        dropped += stop is not None
        early += int(lengths_o[0]) < caps[u]
        n = int(lengths_o[0]) if stop is None else stop + 1
        print(f"utterance {u}: cap {caps[u]} len {len(ids[u])} oracle len {int(lengths_o[0])} step logits {r:.3e} low-gap step {stop}")
        assert ids[u][:n].tolist() == ids_o[0, :n].tolist(), (u, n)
        if stop is None:
            assert len(ids[u]) == int(lengths_o[0])
        assert r <= BAR, (u, r)
    record_figure("decoder_pool_vs_oracle", slots=pc.ORACLE_SLOTS, step_logits_worst=worst, dropped=dropped, ended_by_eos=early)
    assert dropped <= cases.MAX_DROPPED * 12, dropped
    assert early > 0, "no utterance ends by </s>: the refill after an early end is not exercised"


# ---- 2. neighbour independence ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def neighbours(gu):
    model = small_model(gu)
    clips, caps = pc.neighbour_clips(gu.la.synth), pc.NEIGHBOUR_CAPS
    items, out, frames = encode(gu, model, clips, caps)
    assert int(frames.max()) == 1499 and sorted(frames.tolist())[-2] <= 49
    return model, items, out, frames, decode(model, items, 2)


def test_results_do_not_depend_on_the_neighbours(gu, neighbours):
    model, items, _, _, base = neighbours
    assert sorted(base) == list(range(12))
    for k, (ids, lg) in base.items():
        consistent(ids, lg, items[k].cap)
    assert len(base[2][0]) == 300  # the cap-300 row crosses the self-attention's split boundary at 256 keys
    for slots in pc.NEIGHBOUR_SLOTS[1:]:
        assert same(base, decode(model, items, slots)), slots
    assert same(base, decode(model, items[::-1], 5)), "reversed"
    assert same(base, decode(model, items, 5, poll_steps=3)), "another poll rhythm"


# ---- 3. slot hygiene ------------------------------------------------------------------------------------------------------------------
def test_readmitted_slot_and_junk_beyond_frames(gu, neighbours):
    model, items, out, frames, base = neighbours
    long30, short = items[1], items[0]
    assert int(frames[1]) == 1499 and long30.cap == 40 and int(frames[0]) <= 49
    both = decode(model, [long30, short], 1)  # one slot: the 0.3 s clip follows the 30 s clip into it
    alone = decode(model, [short], 1)
    assert torch.equal(both[0][0], alone[0][0]) and torch.equal(both[0][1], alone[0][1])
    assert same(both, {k: base[k] for k in (0, 1)})
    junk = out.clone()
    for b, n in enumerate(frames.tolist()):
        junk[b, n:] = 1e30
    assert same(base, decode(model, rebased(items, junk), 5))


# ---- 4. the contract with generate --------------------------------------------------------------------------------------------------
def test_generate_many_equals_generate_per_pair(gu):
    model = small_model(gu)
    clips, S = pc.oracle_clips(gu.la.synth)[2:8], 12
    batches = batches_of(gu, clips)
    ids, logits = model.generate_many(batches, max_length=S, slots=4, return_logits=True, pack=2)
    dsd, u, worst = _cache["dsd"], 0, 0.0
    for b in batches:
        enc_out, frames = model._encode(b["input_values"], b["attention_mask"])
        want, steps = model.generate(**b, max_length=S, return_logits=True)
        want, steps, lengths = want.cpu(), steps.cpu(), model._decoder_runtime.last_lengths.tolist()
        _, _, lengths_o, gaps = dec_oracle.greedy(enc_out.cpu().double(), frames.cpu().long(), dsd, S)
        stop = cases.first_low_gap_step(gaps, lengths_o)
        for r in range(want.shape[0]):
            n = lengths[r] if stop[r] is None else stop[r] + 1
            assert ids[u][:n].tolist() == want[r, :n].tolist(), (u, n)
            if stop[r] is None:
                assert len(ids[u]) == lengths[r] and bool((want[r, lengths[r]:] == 1).all())
            m = min(n, len(ids[u])) - 1
            if m:
                worst = max(worst, rel_steps(logits[u][:m].cpu(), steps[:m, r]))
            u += 1
    record_figure("decoder_pool_vs_generate", step_logits_worst=worst)
    print("generate_many vs generate: worst step", worst)
    assert u == 6 and worst <= BAR, worst


# ---- 5. limits and the C ABI ----------------------------------------------------------------------------------------------------------
def test_full_pool_single_slot_and_extreme_caps(gu):
    model = small_model(gu)
    clips = [(100 + i, 4800 + 160 * (i % 7)) for i in range(64)]
    caps = [2 + i % 3 for i in range(64)]
    caps[5], caps[6] = 450, 2
    items, _, _ = encode(gu, model, clips, caps)
    full = decode(model, items, 64)
    for k, (ids, lg) in full.items():
        consistent(ids, lg, caps[k])
    assert len(full) == 64 and len(full[6][0]) == 2
    assert len(full[5][0]) == 450 or full[5][0][-1] == 2
    assert same({k: full[k] for k in range(8)}, decode(model, items[:8], 1))
    assert same({k: full[k] for k in range(3)}, decode(model, items[:3], 64))  # a corpus smaller than the pool
    # free and finished slots yield defined values: every row of a step's logits is finite, 61 free slots and one finished included
    dec = importlib.import_module("loco-asr_amd.decoder")
    pool = dec.DecoderPool(model.speecht5.encoder, 64, max(it.rows for it in items), 450, torch.device("cuda", 0))
    pool.submit([items[6], items[5], items[0]])  # caps 2, 450, 2: slots 0 and 2 are finished after the first step
    pool._fill()
    for _ in range(3):
        lg = torch.full((64, 81), float("nan"), device="cuda")
        pool.step(lg)
        assert bool(torch.isfinite(lg).all())
    status, _ = pool.poll()
    assert status[0] == 2 and status[2] == 2 and status[3:] == [0] * 61
    assert model.generate_many([]) == []


def test_two_pools_on_one_handle_interleaved(gu, neighbours):
    model, items, _, _, base = neighbours
    dec = importlib.import_module("loco-asr_amd.decoder")
    a_items, b_items = items[:6], items[6:]
    pools = [dec.DecoderPool(model.speecht5.encoder, 2, 1499, 300, torch.device("cuda", 0), poll_steps=1, return_logits=True) for _ in range(2)]
    pools[0].submit(list(a_items))
    pools[1].submit(list(b_items))
    got = {}
    while pools[0].busy or pools[1].busy:
        for p in pools:  # one step of each in turn
            for k, ids, lg in p.round():
                got[k] = (ids, lg.cpu())
    assert same(got, base)


def test_errors_by_code_and_message(gu, neighbours):
    model, items, out, frames, _ = neighbours
    dec = importlib.import_module("loco-asr_amd.decoder")
    lib, enc, dev0 = gu.lib(), model.speecht5.encoder, torch.device("cuda", 0)
    with pytest.raises(ValueError, match="65 slots exceed the decode step's limit of 64"):
        dec.DecoderPool(enc, 65, 49, 10, dev0)
    with pytest.raises(ValueError, match="S_max = 451"):
        dec.DecoderPool(enc, 2, 49, 451, dev0)
    with pytest.raises(ValueError, match="slots"):
        model.generate_many(batches_of(gu, [(0, 4800)]), slots=65)
    pool = dec.DecoderPool(enc, 2, 49, 10, dev0)
    short = [it for it in items if it.rows <= 49]
    with pytest.raises(ValueError, match="1499 encoder rows.*T_cap = 49"):
        pool.admit([0], [items[1]])
    for cap in (1, 11):
        with pytest.raises(ValueError, match=f"cap {cap}, outside 2 .. S_max = 10"):
            pool.admit([0], [dataclasses.replace(short[0], cap=cap)])
    it = dataclasses.replace(short[0], cap=9)
    pool.admit([0], [it])
    with pytest.raises(gu._libmod.LocoError, match=r"\[-2\].*slot 0 is open"):
        pool.admit([0], [it])
    pool.admit([1], [it])  # the other slot is free
    args = (enc._handle, 2, 49, 10)
    ws = C.c_void_p(pool.workspace.data_ptr())
    assert lib.loco_decoder_pool_step(*args, 0, 49, None, ws, 1024, gu.stream()) == -3
    assert b"workspace 1024 <" in lib.loco_last_error()
    assert lib.loco_decoder_pool_step(*args, 9, 49, None, ws, pool.workspace.numel(), gu.stream()) == -1 and b"position bound" in lib.loco_last_error()
    assert lib.loco_decoder_pool_step(*args, 0, 50, None, ws, pool.workspace.numel(), gu.stream()) == -1 and b"frame bound" in lib.loco_last_error()
    pool.drain()
    bare, _ = gu.model(layers=2)  # an encoder-only handle
    x, m = gu.la.synth.batch([4800])
    bare.speecht5.encoder(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32))
    h = bare.speecht5.encoder._handle
    assert lib.loco_decoder_pool_workspace_bytes(h, 2, 49, 10) == 0
    assert lib.loco_decoder_pool_init(h, 2, 49, 10, ws, pool.workspace.numel(), gu.stream()) == -2 and b"no decoder weights" in lib.loco_last_error()
    torch.cuda.synchronize()


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------------------------
def test_transcribe_slots_writes_the_same_lines(gu, tmp_path, monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = small_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on; 2-layer weights keep it quick
    common = ["--random-init", "--synthetic", "9", "--synthetic-seconds", "1", "--max-length", "3"]
    a, b = tmp_path / "loop.jsonl", tmp_path / "pool.jsonl"
    assert tr.main(common + ["--out", str(a)]) == 0
    assert tr.main(common + ["--slots", "4", "--pack", "2", "--out", str(b)]) == 0
    lines = a.read_text().splitlines()
    assert len(lines) == 9 and [json.loads(l)["id"] for l in lines] == [f"synthetic-{i:06d}" for i in range(9)]
    assert b.read_text() == a.read_text()
