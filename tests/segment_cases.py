"""Inputs of the segmentation tests, shared by tests/test_segment_ref.py (host) and tests/test_gpu_segment.py (-m gpu).  Plain data and
pure helpers; no GPU, no library import."""
import numpy as np

import segment_ref as R

# 100, 20, 5, 5, 3 frames; the noise level is the 2 % quantile so that a signal with a few silent frames still has one
SMALL = dict(max_segment_s=2.0, min_segment_s=0.4, min_silence_s=0.1, min_speech_s=0.1, pad_s=0.06, noise_quantile=0.02)


def two_level(F, speech, low=-80.0, high=-30.0):
    db = np.full(F, low, np.float32)
    for a, b in speech:
        db[a:b] = high
    return db


def edge_cases():
    rng = np.random.default_rng(11)
    out = {}
    out["one_frame"] = (np.array([-30.0], np.float32), dict(SMALL, min_speech_s=0.0))
    out["one_frame_shorter_than_min_speech"] = (np.array([-30.0], np.float32), SMALL)
    out["one_silent_frame"] = (np.array([-90.0], np.float32), SMALL)
    out["all_silence"] = (np.full(300, -90.0, np.float32) + rng.standard_normal(300).astype(np.float32), SMALL)
    out["all_speech_forced_cuts"] = ((-20.0 + rng.standard_normal(3 * 100 + 7)).astype(np.float32), SMALL)
    out["all_speech_equal_energies"] = (np.full(3 * 100 + 7, -20.0, np.float32), SMALL)
    for n in (4, 5):  # min_speech - 1 goes, min_speech stays
        out[f"speech_run_of_{n}"] = (two_level(260, [(10, 70), (90, 90 + n), (120, 200)]), SMALL)
    for n in (4, 5):  # min_silence - 1 is filled, min_silence stays
        out[f"gap_of_{n}"] = (two_level(260, [(10, 60), (60 + n, 130), (150, 250)]), SMALL)
    out["gap_then_short_speech"] = (two_level(260, [(10, 60), (64, 66), (70, 130), (150, 153), (170, 250)]), SMALL)
    out["run_straddles_window_end"] = (two_level(330, [(0, 95), (110, 215), (222, 330)]), SMALL)
    out["run_straddles_window_start"] = (two_level(330, [(0, 15), (30, 230), (236, 330)]), SMALL)
    out["two_equal_runs_in_a_window"] = (two_level(330, [(0, 30), (40, 60), (70, 330)]), SMALL)
    out["silence_at_both_ends"] = (two_level(400, [(130, 270)]), SMALL)
    hostile = R.telegraph(3, 900)
    hostile[::17] = -150.0
    hostile[5::23] = 20.0
    hostile[7::29] = np.nan
    hostile[11::131] = np.inf
    hostile[13::137] = -np.inf
    out["below_-120_above_+8_nan_inf"] = (hostile, SMALL)
    flat = (-20.0 + rng.standard_normal(350)).astype(np.float32)
    flat[3::97] = np.nan  # fewer NaN frames than the noise quantile's rank: peak - noise is small, every other frame is speech
    out["nan_without_usable_silence"] = (flat, SMALL)
    gaps = flat.copy()
    gaps[3::9] = np.nan  # NaN sets the noise level to -120: single silent frames, filled as short gaps
    gaps[200:206] = np.nan
    out["nan_gaps"] = (gaps, SMALL)
    out["all_nan"] = (np.full(250, np.nan, np.float32), SMALL)
    for name, high in (("dynamic_just_under", -35.25), ("dynamic_just_over", -35.0)):  # peak - noise = 14.75 / 15.0 against 15
        out[name] = (two_level(330, [(0, 95), (110, 215), (222, 330)], low=-50.0, high=high), SMALL)
    out["floor_decides"] = (two_level(330, [(0, 95), (110, 215), (222, 330)], low=-90.0, high=-59.75), SMALL)
    out["defaults_short"] = (R.telegraph(5, 2500), {})
    return out


EDGE = edge_cases()


BURSTS = [(8000 + 48000 * k, 40000 + 48000 * k) for k in range(4)]
LONG = dict(max_segment_s=3.5)


def recording():
    rng = np.random.default_rng(2024)
    x = 1e-4 * rng.standard_normal(192000)
    t = np.arange(32000) / 16000.0
    for a, b in BURSTS:
        x[a:b] = 0.1 * np.sin(2 * np.pi * 440.0 * t) + 0.01 * rng.standard_normal(32000)
    return x.astype(np.float32)


# ---- the mono entry's workspace and output contract (tests/test_gpu_segment.py; the names are checked on the host by
# tests/test_segment_ref.py).  F = 1: the smallest recording; 601: the workspace size is no multiple of 16 and there are fewer frames
# than threads; 1025: the first size with two frames per thread and threads past the end; 6001: the walk over cuts takes many steps ----
CONTRACT_F = (1, 601, 1025, 6001)
CONTRACT_PARAMS = dict(max_segment_s=4.0, min_segment_s=0.4)  # 200 frames at most, so that 601 frames are cut at least twice


def contract_inputs(F):
    rng = np.random.default_rng(F)
    return {"silent": (-90.0 + rng.standard_normal(F)).astype(np.float32),  # the path that zeroes the mask
            "all_speech": (-20.0 + rng.standard_normal(F)).astype(np.float32),
            "telegraph": R.telegraph(F, F)}
