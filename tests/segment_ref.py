"""Numpy restatement of the long-form segmentation rules (include/loco_asr.h), written from their text and not from
csrc/segment.hip: plain sequential loops over frames and runs.  Everything that decides a frame, a run or a cut is integer or exact
fp32 arithmetic, so ``segments(db, ...)`` and the device agree bit for bit on the same fp32 ``db`` array."""
import bisect
import math

import numpy as np

HOP, WINDOW, FRAME_RATE = 320, 400, 50
DEFAULTS = dict(max_segment_s=20.0, min_segment_s=1.0, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.2, noise_quantile=0.10,
                peak_quantile=0.99, margin_db=10.0, abs_floor_db=-60.0, min_dynamic_db=15.0, trim=True)


def output_frames(n):
    """The conv stack's chained floors: (n - 80) // 320 for n >= 400."""
    return (n - 80) // HOP if n >= WINDOW else 0


def frame_energy_db(wave):
    """float64: 10 log10(mean(x^2) over samples [320 t, 320 t + 400) + 1e-12)."""
    x = np.asarray(wave, np.float64)
    F = output_frames(x.shape[0])
    idx = HOP * np.arange(F)[:, None] + np.arange(WINDOW)[None, :]
    return 10.0 * np.log10((x[idx] ** 2).mean(axis=1) + 1e-12)


def to_frames(seconds):
    return int(round(seconds * FRAME_RATE))  # ties to even


def bins(db):
    """0.25 dB bins from -120 dB, clamped to 0 .. 511; NaN -> 0."""
    db = np.asarray(db, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((db - np.float32(-120.0)) * np.float32(4.0))
    t = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(511)))
    return t.astype(np.int64)


def threshold(db, noise_quantile, peak_quantile, margin_db, abs_floor_db, min_dynamic_db):
    """(mode, thr): mode "silent" (thr +inf), "all" (thr -inf) or "normal"."""
    F = len(db)
    cum = np.cumsum(np.bincount(bins(db), minlength=512))
    edge = lambda q: np.float32(-120.0) + np.float32(0.25) * np.float32(  # noqa: E731
        int(np.argmax(cum >= min(max(int(math.ceil(q * F)), 1), F))))
    noise, peak = edge(noise_quantile), edge(peak_quantile)
    floor = np.float32(abs_floor_db)
    if peak < floor:
        return "silent", np.float32(np.inf)
    if np.float32(peak - noise) < np.float32(min_dynamic_db):
        return "all", np.float32(-np.inf)
    return "normal", max(floor, np.float32(noise + np.float32(margin_db)))


def runs_of(mask):
    """[(first, end, value)] of the maximal runs of equal values."""
    out, a = [], 0
    for t in range(1, len(mask) + 1):
        if t == len(mask) or mask[t] != mask[a]:
            out.append((a, t, int(mask[a])))
            a = t
    return out


def clean_mask(db, mode, thr, min_silence, min_speech):
    db = np.asarray(db, np.float32)
    with np.errstate(invalid="ignore"):
        mask = (~np.isnan(db) if mode == "all" else db > thr).astype(np.int8)
    rs = runs_of(mask)
    for i, (a, b, v) in enumerate(rs):
        if v == 0 and 0 < i < len(rs) - 1 and b - a < min_silence:
            mask[a:b] = 1
    for a, b, v in runs_of(mask):
        if v == 1 and b - a < min_speech:
            mask[a:b] = 0
    return mask


def order_key(v):
    """fp32 values in the total order NaN < -inf < ... < -0 < +0 < ... < +inf, as an integer."""
    if np.isnan(v):
        return 0
    b = int(np.float32(v).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def cuts(db, mask, max_frames, min_frames):
    """The starts of the segments that tile [0, F): [0, c1, c2, ...]."""
    F = len(db)
    silence = [(a, b) for a, b, v in runs_of(mask) if v == 0]
    firsts, ends = [a for a, _ in silence], [b for _, b in silence]
    out, s = [0], 0
    while F - s > max_frames:
        lo, hi = s + min_frames + 1, s + max_frames  # the next start lies in (s + min, s + max]
        best = None
        for a, b in silence[bisect.bisect_right(ends, lo):bisect.bisect_right(firsts, hi)]:  # the runs that can meet the window
            ca, cb = max(a, lo), min(b, hi + 1)
            if ca < cb and (best is None or cb - ca >= best[1] - best[0]):  # later runs win ties
                best = (ca, cb)
        if best is not None:
            c = (best[0] + best[1]) // 2
        else:
            c = min(range(s + max_frames // 2, hi + 1), key=lambda t: (order_key(db[t]), t))
        out.append(c)
        s = c
    return out


def segments(db, max_segment_s=20.0, min_segment_s=1.0, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.2, noise_quantile=0.10,
             peak_quantile=0.99, margin_db=10.0, abs_floor_db=-60.0, min_dynamic_db=15.0, trim=True, details=False):
    """[(start_frame, end_frame)] (end exclusive) and the threshold; ``details=True``: also the cleaned mask and the untrimmed cuts."""
    db = np.asarray(db, np.float32)
    F = len(db)
    max_frames, min_frames = to_frames(max_segment_s), to_frames(min_segment_s)
    mode, thr = threshold(db, noise_quantile, peak_quantile, margin_db, abs_floor_db, min_dynamic_db)
    if mode == "silent":
        return ([], thr, np.zeros(F, np.int8), []) if details else ([], thr)
    mask = clean_mask(db, mode, thr, to_frames(min_silence_s), to_frames(min_speech_s))
    starts = cuts(db, mask, max_frames, min_frames)
    pad, segs = to_frames(pad_s), []
    for s, c in zip(starts, starts[1:] + [F]):
        if trim:
            speech = np.flatnonzero(mask[s:c])
            if speech.size == 0:
                continue
            segs.append((max(s, s + int(speech[0]) - pad), min(c, s + int(speech[-1]) + 1 + pad)))
        else:
            segs.append((s, c))
    return (segs, thr, mask, starts) if details else (segs, thr)


def telegraph(seed, F, mean_speech=60, mean_silence=25, speech_db=-25.0, silence_db=-75.0, jitter_db=4.0):
    """A seeded random telegraph signal as fp32 db: alternating speech / silence runs of geometric lengths, with level jitter."""
    rng = np.random.default_rng(seed)
    db, t, on = np.empty(F, np.float32), 0, bool(rng.integers(2))
    while t < F:
        n = int(rng.geometric(1.0 / (mean_speech if on else mean_silence)))
        db[t:t + n] = (speech_db if on else silence_db) + jitter_db * rng.standard_normal(min(n, F - t))
        t, on = t + n, not on
    return db
