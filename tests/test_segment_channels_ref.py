"""Properties of the numpy restatement of the per-channel segmentation (tests/segment_channels_ref.py): what the device is compared
against bit for bit must itself do what DESIGN.md 8 says about the cross-talk gate."""
import numpy as np
import pytest

import segment_channels_ref as CR
import segment_ref as R
from segment_cases import EDGE, SMALL
from segment_channels_cases import GRID_PARAMS, PLANTED, grid_db

THRESHOLD_KEYS = ("noise_quantile", "peak_quantile", "margin_db", "abs_floor_db", "min_dynamic_db")


@pytest.mark.parametrize("name", sorted(EDGE))
def test_one_channel_is_the_mono_restatement(name):
    db, params = EDGE[name]
    for gate in (0.0, 15.0, np.inf):
        for trim in (True, False):
            segs, thrs, overlap, masks = CR.segments_channels(db[None], gate, **dict(params, trim=trim))
            want, thr, mask, _ = R.segments(db, details=True, **dict(params, trim=trim))
            assert segs == [want] and len(thrs) == 1 and (thrs[0] == thr or (np.isnan(thrs[0]) and np.isnan(thr)))
            assert (masks[0] == mask).all() and overlap == [[0] * len(want)]


@pytest.mark.parametrize("C", [2, 3])
def test_gate_off_is_the_mono_restatement_per_channel(C):
    db = grid_db(2500, C)
    segs, thrs, overlap, masks = CR.segments_channels(db, np.inf, **GRID_PARAMS)
    for c in range(C):
        want, thr, mask, _ = R.segments(db[c], details=True, **GRID_PARAMS)
        assert segs[c] == want and thrs[c] == thr and (masks[c] == mask).all() and len(want) > 3
        others = np.delete(masks, c, axis=0).any(axis=0)
        assert overlap[c] == [int(others[a:b].sum()) for a, b in want] and sum(overlap[c]) > 0


def test_a_difference_of_exactly_the_gate_is_kept():
    db, params = PLANTED["exact_tie"]
    assert np.float32(db[1, 40] - db[0, 40]) == np.float32(15.0) and np.float32(db[1, 60] - db[0, 60]) > np.float32(15.0)
    g = CR.gated(db, 0, 15.0)
    assert not g[40:60].any() and g[60:80].all() and not g[:40].any() and not g[80:].any()  # 200 .. 229: exactly 15 dB again
    mode, thr = R.threshold(db[0], **{k: dict(R.DEFAULTS, **params)[k] for k in THRESHOLD_KEYS})
    raw = CR.raw_mask(db, 0, mode, thr, 15.0)
    assert raw[20:60].all() and not raw[60:80].any() and raw[80:120].all()
    assert CR.raw_mask(db, 0, mode, thr, np.inf)[20:120].all()
    segs, _, overlap, masks = CR.segments_channels(db, 15.0, **params)
    assert segs[0][0][0] <= 20 and masks[0][60:80].sum() == 0  # 20 gated frames are a pause of min_silence or more: they stay silence


def test_nan_and_missing_others_do_not_gate():
    db, params = PLANTED["nan_and_inf_frames"]
    assert np.isnan(db[1, 500:520]).all() and np.isnan(db[2, 500:520]).all()
    assert not CR.gated(db, 0, 0.0)[500:520].any()
    assert not CR.gated(db[:1], 0, 0.0).any()  # no other channel at all
    assert np.isneginf(db[0, 13]) and np.isneginf(db[1, 13])
    two = db[:2]
    assert not CR.gated(two, 0, 0.0)[13]  # -inf against -inf: a NaN difference is not "greater"
    t = 36  # NaN in channel 0 alone: the others see the maximum of what is left
    assert np.isnan(db[0, t]) and CR.other_max(db, 1)[t] == db[2, t] and CR.other_max(db, 2)[t] == db[1, t]
    lone, lone_params = PLANTED["all_nan_other"]
    segs, _, overlap, _ = CR.segments_channels(lone, 0.0, **lone_params)
    assert segs[0] == R.segments(lone[0], **lone_params)[0] and segs[1] == [] and set(overlap[0]) == {0}


def test_a_silent_channel_yields_nothing_and_stops_nobody():
    db, params = PLANTED["silent_channel"]
    segs, thrs, overlap, masks = CR.segments_channels(db, 15.0, **params)
    assert segs[1] == [] and thrs[1] == np.inf and masks[1].sum() == 0 and overlap[1] == []
    assert len(segs[0]) > 2 and len(segs[2]) > 2 and np.isfinite(thrs[0]) and np.isfinite(thrs[2])
    pair = CR.segments_channels(db[[0, 2]], 15.0, **params)  # its level is below every gate: the others are cut as if it were absent
    assert pair[0] == [segs[0], segs[2]] and pair[2] == [overlap[0], overlap[2]]


def test_identical_channels_and_the_all_speech_mode():
    db, params = PLANTED["identical_channels"]
    segs, _, overlap, _ = CR.segments_channels(db, 0.0, **params)  # 0 > 0 is false: nothing is gated even at 0 dB
    want = R.segments(db[0], **params)[0]
    assert segs == [want] * 3 and overlap[0] == overlap[1] and sum(overlap[0]) > 0
    db, params = PLANTED["all_speech_channel"]
    segs, thrs, _, masks = CR.segments_channels(db, 0.0, **params)
    assert thrs[0] == -np.inf and 0 < masks[0].sum() < db.shape[1]  # all-speech mode is gated too
    assert CR.segments_channels(db, np.inf, **params)[3][0].all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_gate_repairs_a_leaky_pair(seed):
    """Two independent telegraph channels of 6 000 frames, each receiving the other's power at -20 dB.  Against the clean channel's raw
    mask the plain threshold rule is wrong in at least 2 % of the frames, the 15 dB gate in at most 0.5 %."""
    clean, leaky = CR.leaky_pair(seed, 6000, -20.0)
    kw = {k: R.DEFAULTS[k] for k in THRESHOLD_KEYS}
    for c in (0, 1):
        want = CR.raw_mask(clean[c:c + 1], 0, *R.threshold(clean[c], **kw), np.inf)
        mode, thr = R.threshold(leaky[c], **kw)
        plain = int((CR.raw_mask(leaky, c, mode, thr, np.inf) != want).sum())
        gated = int((CR.raw_mask(leaky, c, mode, thr, 15.0) != want).sum())
        print(f"leaky pair seed {seed} channel {c}: {plain} frames wrong ungated, {gated} with the 15 dB gate, of 6000")
        assert plain >= 0.02 * 6000 and gated <= 0.005 * 6000


def test_merged_order_is_start_then_channel():
    segs = [[(5, 9), (20, 30)], [(5, 8), (12, 14)]]
    assert CR.merged(segs, [[1, 2], [3, 4]]) == [(5, 0, 9, 1), (5, 1, 8, 3), (12, 1, 14, 4), (20, 0, 30, 2)]
