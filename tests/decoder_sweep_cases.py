"""Cases of the decoder-against-oracle sweeps, shared by tests/test_gpu_decoder_oracle.py (the library against the oracle, -m gpu)
and tools/decoder_tie_cap.py (the oracle alone on the CPU: how many rows the tie rule would drop).  Plain data and pure helpers; no
GPU, no library import."""
import numpy as np

TIE_GAP = 1e-3      # fixture g13's condition (i): below this relative top-2 gap a correct fp32 decoder may pick the other token
MAX_DROPPED = 0.10  # share of the sweep's rows the tie rule may drop before their end

# (B, S, T_enc, frames or None): loco_decoder_forward against the float64 oracle at every position
TEACHER_FORCED = [
    (1, 1, 1, [1]),                                  # smallest shape
    (2, 2, 64, [64, 63]),                            # key count at 63 / 64
    (3, 65, 257, [257, 256, 1]),                     # key count at 256 / 257, a one-frame clip
    (5, 13, 1499, [1499, 1, 700, 65, 1024]),         # ragged long batch
    (1, 450, 149, None),                             # every position, every encoder row a key (null frame pointer)
    (64, 7, 49, [1 + (11 * b) % 49 for b in range(64)]),  # B at the step's cap, ragged
    (65, 3, 49, [49] * 65),                          # B above 64: lm_head through the skinny kernel with M > 64 rows
    (2, 4, 8192, [8192, 4097]),                      # the teacher-forced cross-attention splits its keys
    (1, 8, 29999, [29999]),                          # ... a 10-minute clip
]
# M = B * S of the fp32 GEMM at and around 64 / 128 / 256: the issue's B in {2, 4, 8} x S = 32 +- 1, and the exact neighbours
TEACHER_FORCED += [(B, S, 23, [23 - (5 * b) % 23 for b in range(B)]) for B in (2, 4, 8) for S in (31, 32, 33)]
TEACHER_FORCED += [(B, S, 9, [9 - b % 9 for b in range(B)]) for B, S in ((1, 63), (1, 65), (1, 127), (3, 43), (5, 51), (1, 257))]
JUNK_CASE = (5, 13, 1499, [1499, 1, 700, 65, 1024])  # repeated with 1e30 in the encoder rows at and beyond frames[b]


def teacher_forced_ids(synth, B, S):
    """Token ids [B, S] in [4, 81) starting with </s>, then, where the row is long enough: <pad> inside rows, the last row of a batch all <pad>
    after position 3, and the vocabulary's ends 0 and 80."""
    ids, _ = synth.token_ids(B, S, seed=17)
    ids[:, 0] = 2
    for b in range(B):
        if S >= 3:
            ids[b, 1 + (3 * b) % (S - 1)] = 1
        if S >= 7 and b % 2 == 0:
            ids[b, 4:6] = 1
    if S >= 5 and B >= 2:
        ids[B - 1, 4:] = 1
    if S >= 2:
        ids[0, S - 1] = 80
    if S >= 4:
        ids[0, 2] = 0
    return ids.astype(np.int64)


def mixed(synth, n, max_samples, seed, min_fraction):
    return synth.mixed_lengths(n, max_samples, seed=seed, min_fraction=min_fraction)


# name -> (decoder seed, clip lengths in samples (a callable of synth), first clip index, max_length).  Seeds 21 / 13 are g13's
# decoder_seed / decoder_seed_c.  With these random weights a row emits </s> either as its first token or not within 450 (of decoder
# seeds 0..178 only three let a row end at all, and then at its first token: tests/golden/make_decoder_goldens.py), so finished
# (<pad>-fed) rows run next to open ones in the mixed batches, and in a batch whose rows all end they all end at step 0: no clip or
# seed was found whose last row ends later than its first.  Under seed 13 every 3 s clip of indices 0..143 ends (short clips mostly
# do not); EARLY_EXIT names the case built from them, where generate must leave its loop at the first poll (after 8 steps, 7 of them
# enqueued past the longest row) and trim to the oracle's width of 2.
GENERATE = {
    "b1_len2": (21, lambda s: [24000], 3, 2),
    "b7_len3_ragged": (13, lambda s: mixed(s, 7, 48000, 3, 0.2), 40, 3),
    "b64_len40_ragged": (13, lambda s: mixed(s, 64, 48000, 5, 0.2), 100, 40),
    "b64_len300_all_end": (13, lambda s: [48000] * 64, 0, 300),
    "b7_len10_all_end": (13, lambda s: [48000] * 7, 64, 10),  # max_length 10: one poll, at the last step but one
    "b7_len40_30s": (13, lambda s: [480000] * 5 + [9000, 12000], 20, 40),  # T_enc = 1499; the two short clips stay open
    "b7_len300_ragged": (13, lambda s: [6000 + 1500 * i for i in range(7)], 60, 300),
    "b2_len300_golden_a_pair": (21, lambda s: [48000, 30400], 0, 300),
    "b1_len450": (13, lambda s: [8000], 2, 450),
}
EARLY_EXIT = ("b64_len300_all_end", "b7_len10_all_end")


def first_low_gap_step(gaps, lengths):
    """Per row: the first step t at which the row is still open (token t + 1 is chosen from logits, t + 1 < lengths[b]) and the
    oracle's relative top-2 gap is below TIE_GAP; None = the row is compared to its end."""
    out = []
    for b in range(gaps.shape[1]):
        hit = None
        for t in range(min(gaps.shape[0], int(lengths[b]) - 1)):
            if float(gaps[t, b]) < TIE_GAP:
                hit = t
                break
        out.append(hit)
    return out
