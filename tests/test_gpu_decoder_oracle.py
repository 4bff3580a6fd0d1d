"""-m gpu: the text decoder (loco_decoder_forward, loco_decoder_generate) against the float64 CPU oracle
oracle/speecht5_decoder_oracle.py, which tests/test_decoder_oracle.py pins to HuggingFace.  Both sides get the same fp32 encoder
output, so only the decoder is measured.  Every comparison is relative L2 against the float64 oracle under the bar the decoder's
goldens already hold, BAR = 2e-5 of tests/test_gpu_decoder.py; the cases are in tests/decoder_sweep_cases.py.

Teacher-forced: logits and all 7 hidden states at every position, over the batch and per clip.
Step path: (a) the oracle teacher-forced on the ids the device produced against the device's step logits, per step and row, finished
rows included; (b) the device's ids against the oracle's own greedy ids under the tie rule of ``check_generate_case``."""
import importlib

import numpy as np
import pytest
import torch

import decoder_sweep_cases as cases
import speecht5_decoder_oracle as dec_oracle
from conftest import golden, record_figure
from test_gpu_decoder import BAR, decoder_forward, full_model  # the bar of the decoder's goldens (2e-5); one cached model per decoder seed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


_sds = {}


def decoder_sd(gu, seed):
    if seed not in _sds:
        _sds[seed] = gu.la.synth.decoder_state_dict(seed)
    return _sds[seed]


def device_forward(gu, model, enc_out, frames, ids):
    logits, hs = decoder_forward(gu, model, enc_out, frames, ids)
    torch.cuda.synchronize()
    return logits.cpu(), [h.cpu() for h in hs]


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def rel_rows(a, b, keep):
    """Worst relative L2 over the slices that keep the first ``keep`` dimensions (per clip: keep = 1; per step and row: keep = 2)."""
    a, b = torch.as_tensor(a).double().flatten(keep), torch.as_tensor(b).double().flatten(keep)
    return float(((a - b).norm(dim=-1) / b.norm(dim=-1)).max())


def tf_inputs(gu, B, S, T, frames):
    synth = gu.la.synth
    enc = (synth.hashed_uniform(f"dec_oracle/enc/{B}/{S}/{T}", (B, T, 768), 2) * np.float32(1.5)).astype(np.float32)
    return enc, cases.teacher_forced_ids(synth, B, S)


# ---- 1. teacher-forced -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,T,frames", cases.TEACHER_FORCED, ids=lambda v: str(v) if isinstance(v, int) else "f")
def test_teacher_forced_against_oracle(gu, g13_seed, B, S, T, frames):
    enc, ids = tf_inputs(gu, B, S, T, frames)
    if S >= 5:
        assert bool((ids[:, 1:] == 1).any()) and ids[0, 2] == 0 and ids[0, S - 1] == 80
        assert B == 1 or bool((ids[B - 1, 4:] == 1).all())
    model = full_model(gu, seed=g13_seed)
    logits, hs = device_forward(gu, model, gu.dev(enc), gu.dev(np.asarray(frames), torch.int32) if frames is not None else None,
                                gu.dev(ids, torch.int32))
    want_hs = []
    want = dec_oracle.forward(enc, frames, ids, decoder_sd(gu, g13_seed), torch.float64, want_hs)
    assert logits.shape == want.shape == (B, S, 81) and len(hs) == len(want_hs) == 7
    r, r_clip = rel(logits, want), rel_rows(logits, want, 1)
    rh = [rel(h, w) for h, w in zip(hs, want_hs)]
    rh_clip = [rel_rows(h, w, 1) for h, w in zip(hs, want_hs)]
    record_figure("decoder_teacher_forced_vs_oracle", B=B, S=S, T_enc=T, frames=None if frames is None else frames[:8], logits=r,
                  logits_worst_clip=r_clip, hidden=rh, hidden_worst_clip=rh_clip)
    print(f"teacher-forced B={B} S={S} T={T}: logits {r:.3e} (worst clip {r_clip:.3e}) hidden {max(rh):.3e} (worst clip {max(rh_clip):.3e})")
    assert bool(torch.isfinite(logits).all())
    assert r <= BAR and r_clip <= BAR, (r, r_clip)
    assert max(rh) <= BAR and max(rh_clip) <= BAR, (rh, rh_clip)


@pytest.fixture(scope="module")
def g13_seed():
    return int(golden("g13_decoder.npz")["decoder_seed"])


def test_encoder_rows_beyond_frames_are_never_read(gu, g13_seed):
    B, S, T, frames = cases.JUNK_CASE
    enc, ids = tf_inputs(gu, B, S, T, frames)
    model = full_model(gu, seed=g13_seed)
    fr, idd = gu.dev(np.asarray(frames), torch.int32), gu.dev(ids, torch.int32)
    logits, hs = device_forward(gu, model, gu.dev(enc), fr, idd)
    junk = enc.copy()
    for b, n in enumerate(frames):
        junk[b, n:] = 1e30
    logits2, hs2 = device_forward(gu, model, gu.dev(junk), fr, idd)
    assert torch.equal(logits, logits2)
    assert all(torch.equal(a, b) for a, b in zip(hs, hs2))


# ---- 2. the step path ----------------------------------------------------------------------------------------------------------
def check_generate_case(gu, name):
    """One case of cases.GENERATE; returns (rows, rows dropped by the tie rule).  (a) step logits: the oracle teacher-forced on the
    device's ids, every step and row.  (b) ids: a row is compared with the oracle's greedy row token by token up to, not including,
    the token chosen at the row's first open step whose oracle top-2 gap is below cases.TIE_GAP, and is dropped from there on; no
    case may drop all its rows, and where none is dropped ids, lengths and trimmed width equal the oracle's."""
    seed, lengths_of, first_index, max_length = cases.GENERATE[name]
    synth = gu.la.synth
    x, m = synth.batch(lengths_of(synth), first_index=first_index)
    model = full_model(gu, seed=seed)
    enc_out, frames = model._encode(gu.dev(x), gu.dev(m, torch.int32))
    ids, steps = model._decoder_runtime.generate(enc_out, frames, max_length, True)
    torch.cuda.synchronize()
    ids, steps, lengths = ids.cpu(), steps.cpu(), model._decoder_runtime.last_lengths.clone()
    enc64, fr = enc_out.cpu().double(), frames.cpu().long()
    B, S = ids.shape
    assert steps.shape == (S - 1, B, 81) and bool(torch.isfinite(steps).all())
    sd = decoder_sd(gu, seed)
    # (a)
    tf = dec_oracle.forward(enc64, fr, ids, sd)[:, :-1]
    got = steps.permute(1, 0, 2)
    ra, ra_worst = rel(got, tf), rel_rows(got, tf, 2)
    # (b)
    ids_o, _, lengths_o, gaps = dec_oracle.greedy(enc64, fr, sd, max_length)
    stop = cases.first_low_gap_step(gaps, lengths_o)
    dropped = sum(t is not None for t in stop)
    record_figure("decoder_generate_vs_oracle", case=name, B=B, max_length=max_length, S=S, T_enc=int(enc_out.shape[1]), step_logits=ra,
                  step_logits_worst_step_row=ra_worst, rows_dropped=dropped, oracle_S=int(ids_o.shape[1]), oracle_lengths=lengths_o.tolist()[:16])
    print(f"generate {name}: B={B} S={S} (oracle {ids_o.shape[1]}, max_length {max_length}) step logits {ra:.3e} (worst step/row {ra_worst:.3e}) "
          f"rows dropped {dropped}")
    assert ra <= BAR and ra_worst <= BAR, (ra, ra_worst)
    assert dropped < B, "the tie rule dropped every row of the case"
    for b in range(B):
        n = min(S, ids_o.shape[1]) if stop[b] is None else stop[b] + 1  # tokens 0 .. stop[b] were chosen before the low-gap step
        assert ids[b, :n].tolist() == ids_o[b, :n].tolist(), (name, b, n)
    if dropped == 0:
        assert S == ids_o.shape[1] and lengths.tolist() == lengths_o.tolist()
        assert ids.tolist() == ids_o.tolist()
    if name in cases.EARLY_EXIT:  # every row ends: the device stops at a poll, discards the steps enqueued past the longest row and trims
        assert dropped == 0 and S == int(lengths_o.max()) < max_length and bool((lengths_o < max_length).all())
        assert max_length >= 10  # so that a poll (every 8 steps) happens before max_length
    return B, dropped


def test_generate_against_oracle(gu):
    """Every case of cases.GENERATE, then the cap over the whole sweep: at most cases.MAX_DROPPED of the rows dropped before their end."""
    rows = dropped = 0
    failures = []
    for name in cases.GENERATE:
        try:
            b, d = check_generate_case(gu, name)
            rows, dropped = rows + b, dropped + d
        except AssertionError as e:  # report every failing case, not only the first
            failures.append(f"{name}: {e}")
    record_figure("decoder_generate_tie_rule", rows=rows, dropped=dropped)
    print("tie rule:", dropped, "of", rows, "rows dropped")
    assert not failures, "\n".join(failures)
    assert dropped <= cases.MAX_DROPPED * rows, (dropped, rows)
