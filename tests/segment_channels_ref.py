"""Numpy restatement of the per-channel segmentation with the cross-talk gate (include/loco_asr.h
"loco_op_vad_segments_channels"), written from their text on top of tests/segment_ref.py: the threshold, the runs, the walk over cuts
and the trim are that module's; what is stated here is the gate at the raw-mask step, the per-channel loop and the overlap count.
Every decision is integer or exact fp32, so ``segments_channels(db, ...)`` and the device agree bit for bit on the same fp32 ``db``."""
import numpy as np

import segment_ref as R


def other_max(db, c):
    """f32 [F]: the maximum of the other channels' values per frame with NaN ignored; NaN where there is none."""
    db = np.asarray(db, np.float32)
    rest = np.delete(db, c, axis=0)
    if rest.shape[0] == 0:
        return np.full(db.shape[1], np.nan, np.float32)
    return np.fmax.reduce(rest, axis=0)


def gated(db, c, crosstalk_db):
    """bool [F]: other(t) - db[c][t] > crosstalk_db in fp32; a frame without another (non-NaN) value is not gated."""
    db = np.asarray(db, np.float32)
    with np.errstate(invalid="ignore"):
        return (other_max(db, c) - db[c]).astype(np.float32) > np.float32(crosstalk_db)  # NaN compares false


def raw_mask(db, c, mode, thr, crosstalk_db):
    """int8 [F]: base(t) && !gated(t); base is db > thr, or "not NaN" in all-speech mode."""
    v = np.asarray(db, np.float32)[c]
    with np.errstate(invalid="ignore"):
        base = ~np.isnan(v) if mode == "all" else v > thr
    return (base & ~gated(db, c, crosstalk_db)).astype(np.int8)


def clean(mask, min_silence, min_speech):
    """The two clean-up passes on a raw mask: interior silence runs shorter than min_silence become speech, then speech runs shorter
    than min_speech become silence."""
    mask = mask.copy()
    rs = R.runs_of(mask)
    for i, (a, b, v) in enumerate(rs):
        if v == 0 and 0 < i < len(rs) - 1 and b - a < min_silence:
            mask[a:b] = 1
    for a, b, v in R.runs_of(mask):
        if v == 1 and b - a < min_speech:
            mask[a:b] = 0
    return mask


def channel(db, c, crosstalk_db, max_segment_s=20.0, min_segment_s=1.0, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.2, noise_quantile=0.10,
            peak_quantile=0.99, margin_db=10.0, abs_floor_db=-60.0, min_dynamic_db=15.0, trim=True):
    """(segments, threshold, cleaned mask) of channel c: the channel's own ungated threshold, the gated mask, the walk, the trim."""
    db = np.asarray(db, np.float32)
    F = db.shape[1]
    mode, thr = R.threshold(db[c], noise_quantile, peak_quantile, margin_db, abs_floor_db, min_dynamic_db)
    if mode == "silent":
        return [], thr, np.zeros(F, np.int8)
    mask = clean(raw_mask(db, c, mode, thr, crosstalk_db), R.to_frames(min_silence_s), R.to_frames(min_speech_s))
    starts = R.cuts(db[c], mask, R.to_frames(max_segment_s), R.to_frames(min_segment_s))
    pad, segs = R.to_frames(pad_s), []
    for s, e in zip(starts, starts[1:] + [F]):
        if trim:
            speech = np.flatnonzero(mask[s:e])
            if speech.size == 0:
                continue
            segs.append((max(s, s + int(speech[0]) - pad), min(e, s + int(speech[-1]) + 1 + pad)))
        else:
            segs.append((s, e))
    return segs, thr, mask


def segments_channels(db, crosstalk_db=15.0, **params):
    """db f32 [C, F] -> (segments per channel, thresholds per channel, overlap per channel, cleaned masks [C, F]).  overlap[c][k] = the
    frames of segment k of channel c in which any other channel's cleaned mask is 1."""
    db = np.asarray(db, np.float32)
    C = db.shape[0]
    per = [channel(db, c, crosstalk_db, **params) for c in range(C)]
    masks = np.stack([m for _, _, m in per])
    overlap = []
    for c in range(C):
        others = np.delete(masks, c, axis=0).any(axis=0) if C > 1 else np.zeros(db.shape[1], bool)
        overlap.append([int(others[a:b].sum()) for a, b in per[c][0]])
    return [p[0] for p in per], [p[1] for p in per], overlap, masks


def merged(segs, overlap):
    """[(start, channel, end, overlap)] in (start, channel) order."""
    return sorted((a, c, b, o) for c, (sc, oc) in enumerate(zip(segs, overlap)) for (a, b), o in zip(sc, oc))


def leaky_pair(seed, F=6000, leak_db=-20.0):
    """The leak experiment: two independent telegraph channels (seeds seed and seed + 100), and the same with each channel receiving
    the other's power at leak_db: (clean f32 [2, F], leaky f32 [2, F])."""
    clean_db = np.stack([R.telegraph(seed, F), R.telegraph(seed + 100, F)]).astype(np.float32)
    p = 10.0 ** (clean_db.astype(np.float64) / 10.0)
    g = 10.0 ** (leak_db / 10.0)
    leaky = 10.0 * np.log10(p + g * p[::-1])
    return clean_db, leaky.astype(np.float32)
