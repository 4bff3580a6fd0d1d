"""g12_attentions.npz is HF's output_attentions=True (tests/golden/make_attention_goldens.py): re-run HF in float64 from the
generator's inputs and check the fixture against it; and the host-only argument errors of the attention-probability ABI."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

_libmod = importlib.import_module("loco-asr_amd._lib")
LOCO_E_INVALID = -1


def test_fixture_matches_hf_float64():
    pytest.importorskip("transformers")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    gen = importlib.import_module("make_attention_goldens")
    fresh = gen.compute()
    g = golden("g12_attentions.npz")
    assert set(g.files) == set(fresh)
    for k in g.files:
        a, b = g[k], fresh[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= 1e-7, k
    # the probabilities themselves: masked keys exactly 0, rows summing to 1
    assert (g["g2_short_rows"][..., 149:] == 0).all()
    assert (g["text_rows"][:, 1, :, :, 31:] == 0).all() and (g["text_rows"][:, 2, :, :, 44:] == 0).all()
    assert np.abs(g["g1_probs"].astype(np.float64).sum(-1) - 1).max() < 1e-5


def test_host_only_argument_errors():
    lib = _libmod.load()
    d = C.c_void_p(16)  # never dereferenced: every call below fails its argument check first
    assert lib.loco_set_attention_outputs(None, None, 0) == LOCO_E_INVALID
    assert lib.loco_op_attention_probs(None, d, None, d, 1, 1, None) == LOCO_E_INVALID
    assert lib.loco_op_attention_probs(d, d, None, None, 1, 1, None) == LOCO_E_INVALID
    assert lib.loco_op_attention_probs_f16x3(d, d, d, d, d, None, d, 1, 1, 4, None) == LOCO_E_INVALID
    assert lib.loco_op_attention_probs_f16x3(d, None, d, d, d, None, d, 1, 1, 3, None) == LOCO_E_INVALID
    assert lib.loco_op_attention_probs_f16x3(d, d, d, d, d, None, d, 1, 1, 1, None) == LOCO_E_INVALID
    assert b"terms" in lib.loco_last_error()


def test_planes_entry_argument_errors():
    """loco_op_attention_f16x3_planes: pe_hi and pe_lo go together, every other pointer is required -- refused on the host, before a launch"""
    lib = _libmod.load()
    d = C.c_void_p(16)  # never dereferenced
    planes = lib.loco_op_attention_f16x3_planes
    ok = [d, d, d, d, d, d, d, d, 1.0, d, None, d, d, 1, 1, None]
    for pe in ((d, None), (None, d)):
        assert planes(*ok[:6], *pe, *ok[8:]) == LOCO_E_INVALID
        assert b"pe_hi and pe_lo" in lib.loco_last_error()
    for missing in (0, 1, 2, 3, 4, 5, 9, 11, 12):  # q, k, v planes, qp, ctx_hi, ctx_lo; with and without pe planes
        for pe in ((d, d), (None, None)):
            args = ok[:6] + list(pe) + ok[8:]
            args[missing] = None
            assert planes(*args) == LOCO_E_INVALID, missing
            assert b"null argument" in lib.loco_last_error()
