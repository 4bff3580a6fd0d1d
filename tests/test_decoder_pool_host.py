"""CPU tests of the decoder pool's host side: the C ABI's answers that need no device, per-utterance caps, generate_many's argument
handling and the position bounds DecoderPool sizes a step by."""
import importlib

import pytest
import torch

la = importlib.import_module("loco-asr_amd")
dec = importlib.import_module("loco-asr_amd.decoder")
_libmod = importlib.import_module("loco-asr_amd._lib")


def test_cabi_host_only_answers():
    lib = _libmod.load()
    assert lib.loco_decoder_pool_workspace_bytes(None, 4, 100, 40) == 0
    for fn, args in (("loco_decoder_pool_init", (None, 4, 100, 40, None, 0, None)),
                     ("loco_decoder_pool_admit", (None, 4, 100, 40, 1, None, None, 0, None, None, None, None, 0, None)),
                     ("loco_decoder_pool_step", (None, 4, 100, 40, 0, 1, None, None, 0, None)),
                     ("loco_decoder_pool_poll", (None, 4, 100, 40, None, None, 0, None)),
                     ("loco_decoder_pool_read", (None, 4, 100, 40, 0, None, None, 0, None))):
        assert getattr(lib, fn)(*args) == -1, fn  # LOCO_E_INVALID: null handle
        assert fn.encode() in lib.loco_last_error() and b"null encoder" in lib.loco_last_error()


def test_caps_per_utterance():
    assert dec.resolve_caps(3, 7) == [7, 7, 7]
    assert dec.resolve_caps(2, None, 4) == [5, 5]
    assert dec.resolve_caps(2) == [dec.DEFAULT_MAX_LENGTH] * 2
    assert dec.resolve_caps(3, [2, 450, 9]) == [2, 450, 9]
    assert dec.resolve_caps(2, torch.tensor([3, 4])) == [3, 4]
    import numpy as np
    assert dec.resolve_caps(2, np.int64(6)) == [6, 6] and dec.resolve_caps(2, np.array([3, 4])) == [3, 4]
    with pytest.raises(ValueError, match="names 2 utterances, the batches hold 3"):
        dec.resolve_caps(3, [2, 3])
    for bad in (1, 451):
        with pytest.raises(ValueError, match="max_length"):
            dec.resolve_caps(2, [5, bad])


def test_generate_many_argument_handling():
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=1)
    for k in ("num_beams", "do_sample", "decoder_input_ids"):
        with pytest.raises(NotImplementedError, match=k):
            model.generate_many([], **{k: 4})
    with pytest.raises(TypeError, match="beams"):
        model.generate_many([], beams=2)
    with pytest.raises(ValueError, match="slots = 65 is outside 1 .. 64"):
        model.generate_many([], slots=65)
    with pytest.raises(ValueError, match="pack"):
        model.generate_many([], pack=0)
    assert model.generate_many([]) == [] and model.generate_many([], return_logits=True) == ([], [])
    with pytest.raises(RuntimeError, match="needs the decoder"):
        la.SpeechT5ForSpeechToTextMI355X(layers=1).generate_many([])


def test_position_bounds_follow_the_steps_enqueued():
    """bounds() = (largest position any slot on the books can be at, most encoder rows, steps until the last cap): exact while a row
    is open, and never beyond cap - 2."""
    pool = dec.DecoderPool.__new__(dec.DecoderPool)
    item = lambda rows, cap: dec.PoolItem(key=0, enc_out=None, frames=None, clip=0, rows=rows, cap=cap)  # noqa: E731
    pool.entries, pool.steps = [(item(49, 3), 0), None, (item(1499, 300), 4)], 4
    assert pool.bounds() == (1, 1499, 299)
    pool.steps = 10
    assert pool.bounds() == (6, 1499, 293)
    pool.entries[2] = None
    assert pool.bounds() == (1, 49, -8)
