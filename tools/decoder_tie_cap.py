#!/usr/bin/env python3
"""CPU check of the tie-rule cap of tests/test_gpu_decoder_oracle.py, oracle alone: for every case of tests/decoder_sweep_cases.py
GENERATE, the float64 encoder oracle's output goes through the decoder oracle's greedy loop, and the rows whose relative top-2 gap
falls below TIE_GAP at an open step are counted.  Exits non-zero when a case would drop all of its rows or the sweep more than
MAX_DROPPED of them.  Prints the CPU time of every case.

    python tools/decoder_tie_cap.py [case ...]
"""
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import decoder_sweep_cases as cases  # noqa: E402
import speecht5_decoder_oracle as dec_oracle  # noqa: E402
import speecht5_oracle as enc_oracle  # noqa: E402

synth = importlib.import_module("loco-asr_amd.synth")


def main():
    names = sys.argv[1:] or list(cases.GENERATE)
    esd = synth.encoder_state_dict(0)
    rows = dropped = 0
    ok = True
    for name in names:
        seed, lengths_of, first_index, max_length = cases.GENERATE[name]
        x, m = synth.batch(lengths_of(synth), first_index=first_index)
        t0 = time.time()
        enc = enc_oracle.encode(x, m, esd, torch.float64)
        frames = enc_oracle.frame_counts(torch.from_numpy(m), enc.shape[1])
        t1 = time.time()
        ids, _, lengths, gaps = dec_oracle.greedy(enc, frames, synth.decoder_state_dict(seed), max_length)
        t2 = time.time()
        stop = cases.first_low_gap_step(gaps, lengths)
        d = sum(t is not None for t in stop)
        rows, dropped = rows + len(stop), dropped + d
        ok = ok and d < len(stop)
        print(f"{name}: B={len(stop)} T_enc={enc.shape[1]} S={ids.shape[1]} lengths {sorted(set(lengths.tolist()))} dropped {d} "
              f"(first low-gap steps {[t for t in stop if t is not None]}) encoder {t1 - t0:.1f} s greedy {t2 - t1:.1f} s", flush=True)
    print(f"rows {rows}, dropped {dropped} ({dropped / rows:.1%}); cap {cases.MAX_DROPPED:.0%}")
    return 0 if ok and dropped <= cases.MAX_DROPPED * rows else 1


if __name__ == "__main__":
    sys.exit(main())
