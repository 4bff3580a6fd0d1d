"""Inputs of the decoder-pool tests, shared by tests/test_gpu_decoder_pool.py (-m gpu) and tools/decoder_pool_tie_cap.py (the oracle
alone on the CPU).  Plain data and pure helpers; no GPU, no library import.

Weights are 2-layer: synth.encoder_state_dict(0, 2) and synth.decoder_state_dict(13, layers=2).  With synthetic weights a row ends
at its first token or never (decoder_sweep_cases.py), so the per-utterance caps are what frees slots at different steps."""
import numpy as np

import decoder_sweep_cases as sweep

ENC_LAYERS, DEC_LAYERS, DEC_SEED = 2, 2, 13


def _from_case(name, take):
    _, lengths_of, first_index, _ = sweep.GENERATE[name]
    return lambda synth: [(first_index + i, n) for i, n in enumerate(lengths_of(synth))][:take]


def oracle_clips(synth):
    """12 clips (clip index, samples) of 0.3 - 3 s: five of GENERATE["b7_len3_ragged"], five of ["b7_len10_all_end"], the shortest
    and an odd length."""
    return _from_case("b7_len3_ragged", 5)(synth) + _from_case("b7_len10_all_end", 5)(synth) + [(7, 4800), (8, 20001)]


ORACLE_CAPS = [2, 3, 5, 9, 4, 17, 2, 6, 11, 3, 40, 8]
ORACLE_SLOTS = 3


def neighbour_clips(synth):
    """12 clips for the bitwise runs: one of 30 s (T_enc = 1499) beside clips of T_enc <= 49, and a row of cap 300 beside rows of cap 3."""
    return [(3, 4800), (4, 480000), (5, 9000), (6, 16000), (9, 5000), (10, 12000), (11, 15999), (12, 7000), (13, 8000), (14, 6400), (15, 16000), (16, 11000)]


NEIGHBOUR_CAPS = [3, 40, 300, 3, 3, 9, 3, 17, 3, 5, 3, 12]
NEIGHBOUR_SLOTS = (2, 5, 64)


def pairs(synth, clips, size=2):
    """The clips as reference batches of ``size``: [(input_values f32 [b, L], attention_mask i32 [b, L])], padded to the longest of
    each batch."""
    out = []
    for b0 in range(0, len(clips), size):
        chunk = clips[b0:b0 + size]
        L = max(n for _, n in chunk)
        x, m = np.zeros((len(chunk), L), np.float32), np.zeros((len(chunk), L), np.int32)
        for i, (index, n) in enumerate(chunk):
            x[i, :n] = synth.clip(index, n)
            m[i, :n] = 1
        out.append((x, m))
    return out
