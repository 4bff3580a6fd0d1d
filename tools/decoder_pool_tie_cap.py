#!/usr/bin/env python3
"""CPU check of the tie-rule cap of tests/test_gpu_decoder_pool.py, oracle alone: the 12 utterances of tests/decoder_pool_cases.py go
pair by pair through the float64 encoder oracle and one by one, each with its own cap, through the decoder oracle's greedy loop; the
utterances whose relative top-2 gap falls below TIE_GAP at an open step are counted.  Exits non-zero when more than MAX_DROPPED of
them would be cut short.

    python tools/decoder_pool_tie_cap.py
"""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import decoder_pool_cases as pool_cases  # noqa: E402
import decoder_sweep_cases as cases  # noqa: E402
import speecht5_decoder_oracle as dec_oracle  # noqa: E402
import speecht5_oracle as enc_oracle  # noqa: E402

synth = importlib.import_module("loco-asr_amd.synth")


def main():
    esd = synth.encoder_state_dict(0, pool_cases.ENC_LAYERS)
    dsd = synth.decoder_state_dict(pool_cases.DEC_SEED, layers=pool_cases.DEC_LAYERS)
    caps = pool_cases.ORACLE_CAPS
    u = dropped = 0
    for x, m in pool_cases.pairs(synth, pool_cases.oracle_clips(synth)):
        enc = enc_oracle.encode(x, m, esd, torch.float64)
        frames = enc_oracle.frame_counts(torch.from_numpy(m), enc.shape[1])
        for b in range(x.shape[0]):
            ids, _, lengths, gaps = dec_oracle.greedy(enc[b:b + 1], frames[b:b + 1], dsd, caps[u])
            stop = cases.first_low_gap_step(gaps, lengths)[0]
            dropped += stop is not None
            print(f"utterance {u}: frames {int(frames[b])} cap {caps[u]} length {int(lengths[0])} ids {ids[0].tolist()[:8]} "
                  f"min gap {float(gaps.min()):.2e} first low-gap step {stop}", flush=True)
            u += 1
    print(f"utterances {u}, dropped {dropped} ({dropped / u:.1%}); cap {cases.MAX_DROPPED:.0%}")
    return 0 if dropped <= cases.MAX_DROPPED * u else 1


if __name__ == "__main__":
    sys.exit(main())
