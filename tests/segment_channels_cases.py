"""Inputs of the per-channel segmentation tests, shared by tests/test_segment_channels_ref.py (host) and
tests/test_gpu_segment_channels.py (-m gpu).  Plain data and pure helpers; no GPU, no library import."""
import numpy as np

import segment_ref as R
from segment_cases import SMALL, two_level

GRID_F = (1, 2, 1023, 1024, 1025, 6000, 20000)  # around the workgroup's 1024 threads, then many frames per thread
GRID_C = (1, 2, 3)
GATES = (0.0, 15.0, float("inf"))
GRID_PARAMS = dict(max_segment_s=4.0, min_segment_s=0.4)  # 200 frames at most: the walk takes up to a hundred steps


def leaky(clean_db, leak_db=-20.0):
    """Every channel receives the summed power of the others at leak_db; fp32 [C, F]."""
    p = 10.0 ** (np.asarray(clean_db, np.float64) / 10.0)
    return (10.0 * np.log10(p + 10.0 ** (leak_db / 10.0) * (p.sum(axis=0, keepdims=True) - p))).astype(np.float32)


def grid_db(F, C):
    """C telegraph channels of F frames with -20 dB leak; C == 1: the plain telegraph signal."""
    return leaky(np.stack([R.telegraph(1000 * C + 7 * c + F % 97, F) for c in range(C)]))


def planted_cases():
    out = {}
    # a difference of exactly 15 dB is kept, the next fp32 value above it is gated: frames 40 .. 79 of channel 0
    a = two_level(300, [(20, 120), (180, 260)], high=-40.0)
    b = two_level(300, [(40, 80), (200, 230)], low=-90.0, high=-25.0)
    b[60:80] = np.nextafter(np.float32(-25.0), np.float32(0.0))
    out["exact_tie"] = (np.stack([a, b]), SMALL)
    hostile = leaky(np.stack([R.telegraph(3, 900), R.telegraph(4, 900), R.telegraph(5, 900)]))
    hostile[0, 7::29] = np.nan
    hostile[1, 7::31] = np.nan
    hostile[2, 5::37] = np.nan
    hostile[0, 13::137] = -np.inf
    hostile[1, 13::41] = -np.inf  # frame 13: -inf in both, a NaN difference
    hostile[2, 11::131] = np.inf
    hostile[1, 500:520] = np.nan
    hostile[2, 500:520] = np.nan  # every other channel NaN: channel 0 is not gated there
    out["nan_and_inf_frames"] = (hostile, SMALL)
    one = R.telegraph(8, 700)
    out["identical_channels"] = (np.stack([one, one, one]), SMALL)
    rng = np.random.default_rng(12)
    quiet = (-90.0 + rng.standard_normal(700)).astype(np.float32)
    out["silent_channel"] = (np.stack([R.telegraph(9, 700), quiet, R.telegraph(10, 700)]), SMALL)
    flat = (-20.0 + rng.standard_normal(700)).astype(np.float32)
    out["all_speech_channel"] = (np.stack([flat, R.telegraph(11, 700, speech_db=-10.0)]), SMALL)
    out["all_nan_other"] = (np.stack([R.telegraph(12, 400), np.full(400, np.nan, np.float32)]), SMALL)
    return out


PLANTED = planted_cases()


# ---- the synthetic two-channel call of the end-to-end tests ----
CALL_SECONDS = 24
# (channel, first sample, end sample) of the bursts: A and B alternate, the third pair overlaps.  No burst is longer than 3 s, so that
# with max_segment_s = 4 a window of the walk that starts in the pause before a burst always reaches the pause behind it
CALL_BURSTS = [(0, 16000, 56000), (1, 72000, 112000), (0, 128000, 168000), (1, 184000, 224000), (0, 240000, 288000), (1, 264000, 312000)]
CALL_VAD = dict(max_segment_s=4.0)
CALL_LEAK_DB = -25.0
