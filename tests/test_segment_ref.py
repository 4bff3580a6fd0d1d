"""Properties of the numpy restatement of the segmentation rules (tests/segment_ref.py) on seeded random telegraph signals: what the
device is later compared against bit for bit must itself do what DESIGN.md 8 says."""
import numpy as np
import pytest

import segment_ref as R
from segment_cases import CONTRACT_F, CONTRACT_PARAMS, EDGE, LONG, contract_inputs, recording

# (seed, F, parameters): short maxima so that every signal is cut many times; one case without any usable silence
CASES = [(seed, 1500 + 217 * seed, dict(max_segment_s=2.0 + 0.5 * (seed % 5), min_segment_s=0.2 + 0.1 * (seed % 3),
                                         min_silence_s=0.1 + 0.1 * (seed % 3), min_speech_s=0.1, pad_s=0.1 * (seed % 3)))
         for seed in range(12)]


def windows(starts, F, max_frames, min_frames):
    """(s, c, lo, hi) of every cut c made from s."""
    return [(s, c, s + min_frames + 1, s + max_frames) for s, c in zip(starts, starts[1:])]


@pytest.mark.parametrize("seed,F,params", CASES)
def test_segments_are_ordered_disjoint_and_bounded(seed, F, params):
    db = R.telegraph(seed, F)
    for trim in (True, False):
        segs, _ = R.segments(db, trim=trim, **params)
        assert segs
        prev = 0
        for a, b in segs:
            assert prev <= a < b <= F
            assert b - a <= R.to_frames(params["max_segment_s"])
            prev = b


@pytest.mark.parametrize("seed,F,params", CASES)
def test_untrimmed_segments_tile_the_recording(seed, F, params):
    segs, _ = R.segments(R.telegraph(seed, F), trim=False, **params)
    assert segs[0][0] == 0 and segs[-1][1] == F
    assert all(b == a2 for (_, b), (a2, _) in zip(segs, segs[1:]))


@pytest.mark.parametrize("seed,F,params", CASES)
def test_trimmed_segments_keep_every_speech_frame(seed, F, params):
    segs, _, mask, _ = R.segments(R.telegraph(seed, F), trim=True, details=True, **params)
    covered = np.zeros(F, bool)
    for a, b in segs:
        covered[a:b] = True
    assert mask.sum() > 0 and covered[mask == 1].all()
    pad = R.to_frames(params["pad_s"])
    for a, b in segs:  # no more than pad frames of silence at either end, unless the cut is nearer
        assert mask[a:b].any()
        first, last = a + int(np.argmax(mask[a:b])), b - 1 - int(np.argmax(mask[a:b][::-1]))
        assert first - a <= pad and b - 1 - last <= pad


@pytest.mark.parametrize("seed,F,params", CASES)
def test_cuts_fall_in_silence_whenever_the_window_holds_some(seed, F, params):
    db = R.telegraph(seed, F)
    _, _, mask, starts = R.segments(db, details=True, **params)
    maxf, minf = R.to_frames(params["max_segment_s"]), R.to_frames(params["min_segment_s"])
    assert len(starts) > 3
    for s, c, lo, hi in windows(starts, F, maxf, minf):
        if (mask[lo:hi + 1] == 0).any():
            assert lo <= c <= hi and mask[c] == 0
        else:
            assert s + maxf // 2 <= c <= hi
            assert db[c] == db[s + maxf // 2:hi + 1].min()


def test_forced_cuts_without_silence():
    """All speech: peak - noise < min_dynamic_db, the threshold is -inf and every cut is the first least-energy frame of its window."""
    rng = np.random.default_rng(5)
    db = (-20 + rng.standard_normal(3 * 100 + 7)).astype(np.float32)
    segs, thr, mask, starts = R.segments(db, max_segment_s=2.0, min_segment_s=0.5, details=True)
    assert thr == -np.inf and mask.all() and len(starts) >= 3
    for s, c in zip(starts, starts[1:]):
        assert c == s + 50 + int(np.argmin(db[s + 50:s + 101]))
    assert segs[0][0] == 0 and segs[-1][1] == len(db)


def test_threshold_rules():
    silent = np.full(200, -90.0, np.float32)
    assert R.segments(silent) == ([], np.float32(np.inf))
    db = np.full(200, -80.0, np.float32)
    db[50:150] = -30.0
    segs, thr = R.segments(db)
    assert thr == np.float32(-60.0) and segs == [(40, 160)]  # noise -80 + 10 is below the floor; pad 10 frames
    db[:50] = db[150:] = -50.0
    assert R.segments(db)[1] == np.float32(-40.0)
    assert R.bins(np.array([np.nan, -130.0, -120.0, -119.75, 7.9, 8.0, np.inf, -np.inf], np.float32)).tolist() == [0, 0, 0, 1, 511, 511, 511, 0]
    assert R.to_frames(0.3) == 15 and R.to_frames(0.25) == 12 and R.to_frames(0.27) == 14


def test_edge_cases_do_what_their_names_say():
    """On the host's restatement (no device): the cases above reach the rules they are named after."""
    seg_of = lambda name, **kw: R.segments(EDGE[name][0], **dict(EDGE[name][1], **kw), details=True)  # noqa: E731
    assert seg_of("one_frame")[0] == [(0, 1)] and seg_of("one_frame_shorter_than_min_speech")[0] == []
    assert seg_of("all_silence")[1] == np.inf and seg_of("all_speech_forced_cuts")[1] == -np.inf
    assert len(seg_of("all_speech_forced_cuts")[3]) >= 4 and seg_of("all_speech_equal_energies")[3][:3] == [0, 50, 100]
    assert seg_of("speech_run_of_4")[2][90:94].sum() == 0 and seg_of("speech_run_of_5")[2][90:95].sum() == 5
    assert seg_of("gap_of_4")[2][60:64].sum() == 4 and seg_of("gap_of_5")[2][60:65].sum() == 0
    assert seg_of("run_straddles_window_end")[3][1] == (95 + 101) // 2  # [95, 110) clipped to the window (20, 100]
    assert seg_of("two_equal_runs_in_a_window")[3][1] == 65  # [30, 40) and [60, 70): the later run
    assert seg_of("dynamic_just_under")[1] == -np.inf and seg_of("dynamic_just_over")[1] == np.float32(-40.0)
    assert seg_of("floor_decides")[1] == np.float32(-60.0)


def test_recording_by_the_rules_on_the_host():
    """Before any GPU run: the restatement on the float64 energies gives thr = -60 dB, the cuts derived in the module docstring and
    four segments of one burst each."""
    segs, thr, mask, starts = R.segments(R.frame_energy_db(recording()).astype(np.float32), details=True, **LONG)
    assert thr == np.float32(-60.0) and starts == [0, 149, 299, 449]
    assert segs == [(14, 135), (164, 285), (314, 435), (464, 585)]
    assert [(a, b) for a, b, v in R.runs_of(mask) if v == 0][1:4] == [(125, 174), (275, 324), (425, 474)]


@pytest.mark.parametrize("F", CONTRACT_F)
def test_contract_inputs_are_what_their_names_say(F):
    """The inputs of the mono entry's workspace contract test on the device: silent, without usable silence, cut more than once."""
    dbs = contract_inputs(F)
    segs, thr = R.segments(dbs["silent"], **CONTRACT_PARAMS)
    assert segs == [] and thr == np.inf
    segs, thr = R.segments(dbs["all_speech"], **CONTRACT_PARAMS)
    assert thr == -np.inf and (F < 601 or len(segs) >= 2)
    segs, thr = R.segments(dbs["telegraph"], **CONTRACT_PARAMS)
    assert F < 601 or (len(segs) >= 2 and np.isfinite(thr))
